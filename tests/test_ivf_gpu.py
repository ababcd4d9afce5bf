"""The range scan, the top-k merge, the k-means accumulation and the IVF index on the GPU, each
against an exact oracle: fp64 scores of the bf16 operands, a plain Python sort, fp64 sums.

Tolerance of a score, TOL: the range scan adds d <= 4096 exact bf16 x bf16 products in fp32; with unit
rows and queries (sum |x_i q_i| <= 1) that is at most d * 2^-24 ~ 2.4e-4 from the exact sum, and far
less in practice. TOL is 4 x the largest |kernel - fp64| measured over every case of this file.
A row whose exact score lies within TOL of a similarity floor may fall on either side of it.

rows_per_split = 200 (no multiple of the kernel's 64-row step) needs no limit: the scan walks
positions [lo, hi) of a split in steps of 64 and masks the tail, whatever the split length.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from docagents_amd.index.flat import FlatIndex  # noqa: E402
from docagents_amd.index.ivf import IVFFlatIndex  # noqa: E402
from docagents_amd.ops import kernels as K  # noqa: E402

from topk_cases import MERGE_K, MERGE_P, MERGE_Q, assert_merge, merge_case  # noqa: E402

DEV = "cuda"
BF16 = torch.bfloat16
TOL = 7.1e-7     # 4 x 1.77e-7, the largest |kernel - fp64| over all 92 cases of this file on an MI355X
MAX_ERR = [0.0]   # largest |returned score - fp64 score| seen by _assert_topk in this process


def _unit(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=-1)


def _np(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------ exactness helper
def _assert_topk(got_s, got_i, scores64, allowed, K, tol):
    """One query's result row against the fp64 scores of every row (``scores64``) and the rows the
    query may return (``allowed``, bool)."""
    s, i = np.asarray(got_s, dtype=np.float64), np.asarray(got_i, dtype=np.int64)
    assert s.shape == (K,) and i.shape == (K,)
    real = i >= 0
    ids = i[real]
    assert len(set(ids.tolist())) == ids.size, f"a row came back twice: {i.tolist()}"
    assert bool(((i == -1) == np.isneginf(s)).all()) and bool((i >= -1).all()), (i.tolist(), s.tolist())
    assert bool((ids < allowed.size).all()) and bool(allowed[ids].all()), "a row outside the allowed set came back"
    n_real = min(K, int(allowed.sum()))
    assert int(real.sum()) == n_real, f"{int(real.sum())} rows returned, {n_real} expected"
    err = float(np.abs(s[real] - scores64[ids]).max(initial=0.0))
    MAX_ERR[0] = max(MAX_ERR[0], err)
    assert err <= tol, f"score error {err:.3g} > {tol:.3g}"
    for a in range(K - 1):  # descending; equal scores by ascending id; the padding last
        assert s[a] > s[a + 1] or (s[a] == s[a + 1] and (i[a] < i[a + 1] or i[a] == i[a + 1] == -1)), \
            (a, s.tolist(), i.tolist())
    if n_real:
        exact_kth = np.sort(scores64[allowed])[::-1][n_real - 1]
        assert s[n_real - 1] >= exact_kth - tol, f"k-th score {s[n_real - 1]} < exact k-th {exact_kth}: a better row was dropped"


def _floored(scores64, allowed, thr, got_i, tol):
    """``allowed`` under a similarity floor: rows at or above it, where a row within tol of the floor
    counts exactly if it was returned."""
    got = np.asarray(got_i, dtype=np.int64)
    got = got[got >= 0]
    assert bool((got < allowed.size).all())
    ret = np.zeros(allowed.size, dtype=bool)
    ret[got] = True
    return allowed & np.where(np.abs(scores64 - thr) <= tol, ret, scores64 >= thr)


def _check_rows(got, S, allowed, Kk, thr=None):
    s, i = _np(got[0]), _np(got[1])
    assert s.shape == (S.shape[0], Kk) and s.dtype == np.float32 and i.dtype == np.int32
    for q in range(S.shape[0]):
        al = allowed[q] if thr is None else _floored(S[q], allowed[q], thr, i[q], TOL)
        _assert_topk(s[q], i[q], S[q], al, Kk, TOL)
        if thr is not None:
            assert bool((s[q][i[q] >= 0] >= thr).all())
    return s, i


# ------------------------------------------------------------------------------------------ topk_ranges
RN, RQ = 3000, 6
_RANGES = {}


def _ranges_data(d):
    """Rows, queries (on the GPU) and their fp64 scores, once per d. Rows 40..49 and 2000..2009 are
    bit-identical copies of one row."""
    if d not in _RANGES:
        X = _unit(RN, d, d).to(BF16)
        X[40:50] = X[40]
        X[2000:2010] = X[40]
        Qv = _unit(RQ, d, d + 1)
        Qv[1] = -(X[5].float() + X[2999].float())            # both of query 1's rows score below zero
        Qv[3] = X[1500].float()                              # query 3 (every row) finds row 1500 at ~1
        Qv = torch.nn.functional.normalize(Qv, dim=-1).to(BF16)
        S = (Qv.double() @ X.double().t()).numpy()
        _RANGES[d] = (X.to(DEV).contiguous(), Qv.to(DEV).contiguous(), S)
    return _RANGES[d]


def _table(r):
    """Six queries' ranges for rows_per_split = r. Positions count rows along a query's concatenated
    ranges; split s covers positions [s r, (s + 1) r)."""
    return [
        # 0: r - 10 rows; then 30 rows straddling the boundary at position r (and in descending row
        #    order); then r - 20 rows ending exactly on the boundary 2 r; then a single row opening split 2
        [(2400, 2400 + r - 10), (100, 130), (1000, 1000 + r - 20), (7, 8)],
        [(5, 6), (2999, 3000)],                              # 1: two single rows: fewer than K = 6, 32
        [],                                                  # 2: no ranges, between two queries that have some
        [(0, RN)],                                           # 3: every row: max_rows
        [(2900, 2990), (1500, 1777), (300, 301), (0, 64)],   # 4: descending, odd lengths, the ten copies
        [(123, 123 + 3 * r + 17)],                           # 5: one range over four splits
    ]


def _range_tensors(table, n=RN):
    rg = [list(ab) for t in table for ab in t]
    ro = np.cumsum([0] + [len(t) for t in table])
    allowed = np.zeros((len(table), n), dtype=bool)
    for q, t in enumerate(table):
        for a, b in t:
            assert 0 <= a < b <= n and not allowed[q, a:b].any()
            allowed[q, a:b] = True
    ranges = torch.tensor(rg, dtype=torch.int32, device=DEV).reshape(-1, 2).contiguous()
    return ranges, torch.tensor(ro, dtype=torch.int32, device=DEV), allowed


@pytest.mark.parametrize("rps", [64, 200, 512])
@pytest.mark.parametrize("Kk", [1, 6, 32])
@pytest.mark.parametrize("d", [8, 264, 768, 4096])
def test_topk_ranges_exact(d, Kk, rps):
    """d: 1 chunk, 33 chunks (one past the 32-lane stride), 96, all 16 x 32 register chunks.
    rows_per_split 200 is no multiple of the kernel's 64-row step."""
    X, Qv, S = _ranges_data(d)
    ranges, roff, allowed = _range_tensors(_table(rps))
    assert int(allowed.sum(1).max()) == RN
    kw = dict(max_rows=RN, rows_per_split=rps)
    _check_rows(K.topk_ranges(X, Qv, ranges, roff, Kk, -2.0, **kw), S, allowed, Kk)
    # a floor: removes some of query 3's rows and every row of query 1
    thr = 0.5
    s, i = _check_rows(K.topk_ranges(X, Qv, ranges, roff, Kk, thr, **kw), S, allowed, Kk, thr=thr)
    assert int(i[3, 0]) == 1500 and not bool((i[1] >= 0).any())
    assert 0 < int((S[3] >= thr + TOL).sum()) < RN and not bool((S[1][allowed[1]] >= thr - TOL).any())
    # slots (some -1) and a bitmap of W = 6 words: slots 192.. (rows 1920..) lie past it and never match
    W = 6
    slots = (torch.arange(RN, dtype=torch.int32) // 10)
    slots[::7] = -1
    bits = np.random.default_rng(d + Kk).integers(0, 1 << 32, (RQ, W), dtype=np.uint64).astype(np.uint32)
    bitmap = torch.from_numpy(bits.view(np.int32)).to(DEV).contiguous()
    sl = slots.numpy().astype(np.int64)
    word = np.clip(sl >> 5, 0, W - 1)
    ok = (sl >= 0) & ((sl >> 5) < W) & (((bits[:, word] >> (sl & 31).astype(np.uint32)) & 1) == 1)
    assert bool(ok[:, :1920].any()) and not bool(ok[:, 1920:].any()) and int((sl >> 5).max()) >= W
    s, i = _check_rows(K.topk_ranges(X, Qv, ranges, roff, Kk, -2.0, slots=slots.to(DEV), bitmap=bitmap, **kw),
                       S, allowed & ok, Kk)
    assert not bool((i >= 1920).any()) and not bool(((i >= 0) & (i % 7 == 0)).any())
    # slots alone: removed rows only
    _check_rows(K.topk_ranges(X, Qv, ranges, roff, Kk, -2.0, slots=slots.to(DEV), **kw), S,
                allowed & (sl >= 0)[None, :], Kk)


@pytest.mark.parametrize("rps", [64, 200, 512])
@pytest.mark.parametrize("Kk", [1, 6, 32])
def test_topk_ranges_ties(Kk, rps):
    """20 bit-identical copies of one row in two ranges that land in different splits, queried with
    that row: exactly the K smallest ids among the copies, whichever split or range they sit in."""
    X, _, _ = _ranges_data(264)
    Qv = torch.stack([X[40], X[77]]).contiguous()
    table = [[(1950, 2010), (500, 500 + 2 * rps), (30, 60)],   # copies at positions 50..59 and 2 rps + 70..79
             [(0, RN)]]
    ranges, roff, allowed = _range_tensors(table)
    S = (Qv.double().cpu() @ X.double().cpu().t()).numpy()
    s, i = _check_rows(K.topk_ranges(X, Qv, ranges, roff, Kk, -2.0, max_rows=RN, rows_per_split=rps), S, allowed, Kk)
    copies = list(range(40, 50)) + list(range(2000, 2010))
    assert i[0, :20].tolist() == copies[:Kk]
    assert bool((s[0, :min(Kk, 20)] == s[0, 0]).all())


# ------------------------------------------------------------------------------------------- topk_merge
@pytest.mark.parametrize("Kk", MERGE_K)
@pytest.mark.parametrize("Q", MERGE_Q)
@pytest.mark.parametrize("P", MERGE_P)
def test_topk_merge_exact(P, Q, Kk):
    cs, ci = merge_case(P, Q, Kk)
    cs, ci = cs.to(DEV), ci.to(DEV)
    keep_s, keep_i = cs.clone(), ci.clone()
    s, i = K.topk_merge(cs, ci, Kk)
    torch.cuda.synchronize()
    assert_merge(s, i, keep_s, keep_i, Kk)
    assert torch.equal(cs.view(torch.int32), keep_s.view(torch.int32)) and torch.equal(ci, keep_i), \
        "topk_merge changed the caller's candidates"


# ----------------------------------------------------------------------------------------- kmeans_accum
U = 2.0 ** -24   # fp32 unit roundoff


def _accum_check(X, assign, s0, c0):
    """sums / counts after the kernel against fp64. An element that receives m terms (its non-zero
    start value counts as one) is the result of m - 1 rounded fp32 additions in some order; each
    rounds by at most U x |partial sum| <= U x sum |terms|, so whatever the order
    |got - exact| <= (m - 1) U sum|terms| / (1 - (m - 1) U). bf16 -> fp32 is exact. The fp64 oracle
    itself is within m 2^-53 sum|terms|."""
    L, d = s0.shape
    sums, counts = s0.clone(), c0.clone()
    K.kmeans_accum(X, assign, sums, counts)
    torch.cuda.synchronize()
    a = assign.long()
    m = a >= 0
    n_c = torch.bincount(a[m], minlength=L)
    assert torch.equal(counts, c0 + n_c.float()), "counts"
    exact, absum = s0.double(), s0.double().abs()
    exact.index_add_(0, a[m], X[m].double())
    absum.index_add_(0, a[m], X[m].double().abs())
    terms = n_c.double()[:, None] + (s0 != 0).double()
    adds = (terms - 1).clamp_min(0)
    bound = adds * U * absum / (1 - adds * U) + terms * 2.0 ** -53 * absum
    over = (sums.double() - exact).abs() - bound
    assert float(over.max()) <= 0, f"sum error {float(over.max()):.3g} above the summation bound"
    idle = n_c == 0
    assert torch.equal(sums.view(torch.int32)[idle], s0.view(torch.int32)[idle]), "a list that got no row changed"
    return n_c


@pytest.mark.parametrize("L", [1, 10, 300])
@pytest.mark.parametrize("N,d", [(1, 8), (700, 100), (5000, 768), (3000, 1024)])
def test_kmeans_accum_exact(N, d, L):
    g = torch.Generator().manual_seed(N + d + L)
    X = torch.randn(N, d, generator=g).to(BF16).to(DEV).contiguous()
    zero_s, zero_c = torch.zeros(L, d, device=DEV), torch.zeros(L, device=DEV)
    # onto non-zero sums and counts (with a -0.0 and a denormal that only survive untouched)
    s0 = torch.randn(L, d, generator=g).to(DEV)
    s0[L - 1, 0], s0[L - 1, d - 1] = -0.0, 1e-41
    c0 = torch.randint(0, 9, (L,), generator=g).float().to(DEV)
    assign = torch.randint(-1, L, (N,), generator=g, dtype=torch.int32).to(DEV)
    if N > 1:
        assign[assign == L - 1] = -1                      # list L - 1 gets no row (L = 1: no row at all)
    n_c = _accum_check(X, assign, s0, c0)
    assert N == 1 or int(n_c[L - 1]) == 0
    # every row into one list: every atomic of a column lands on one address
    n_c = _accum_check(X, torch.full((N,), L - 1, dtype=torch.int32, device=DEV), zero_s, zero_c)
    assert int(n_c[L - 1]) == N
    # nothing assigned: nothing changes
    sums, counts = s0.clone(), c0.clone()
    K.kmeans_accum(X, torch.full((N,), -1, dtype=torch.int32, device=DEV), sums, counts)
    torch.cuda.synchronize()
    assert torch.equal(sums.view(torch.int32), s0.view(torch.int32)) and torch.equal(counts, c0)


# ------------------------------------------------------------------------------------------------- IVF
# dim 768, n 6000: the GEMM + argmax assignment (n >= 4096, dim % 64 == 0) and the streaming centroid
# scan; dim 96, n 2000: the topk_dense assignment (n < 4096) and the query-major centroid scan. The
# centroid scans (topk_dense) need dim % 32 == 0: an IVF index on the GPU cannot run at dim 72
# (test_ivf_needs_dim_multiple_of_32).
GEOMS = {"gemm768": (768, 6000), "dense96": (96, 2000)}
LISTS = 16
_IVF = {}


def _clustered(n, dim, seed):
    g = torch.Generator().manual_seed(seed)
    C = torch.nn.functional.normalize(torch.randn(12, dim, generator=torch.Generator().manual_seed(dim)), dim=-1)
    x = C[torch.randint(0, 12, (n,), generator=g)] + 0.5 * torch.nn.functional.normalize(
        torch.randn(n, dim, generator=g), dim=-1)
    return torch.nn.functional.normalize(x, dim=-1).to(BF16)


class _Corpus:
    """The vectors as added (insertion order j), their external ids and documents; the oracle of a
    search in the index's row space, reached through ids_t alone."""

    def __init__(self, dim, n):
        self.dim = dim
        self.V = _clustered(n, dim, n)
        self.ext = np.random.default_rng(n).permutation(n).astype(np.int64) * 16661 + 5   # up to ~1e8
        cuts = [0, int(.15 * n), int(.16 * n), int(.45 * n), int(.45 * n) + 1, int(.8 * n), n]
        self.doc = np.zeros(n, dtype=np.int64)
        self.names = [f"doc{i}" for i in range(len(cuts) - 1)]
        for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            self.doc[a:b] = i
        self.removed = set()

    def extend(self, name, rows, seed):
        n0 = self.V.shape[0]
        self.V = torch.cat([self.V, _clustered(rows, self.dim, seed)])
        self.ext = np.concatenate([self.ext, 10 ** 8 + seed * 10 ** 4 + np.arange(rows, dtype=np.int64)])
        self.doc = np.concatenate([self.doc, np.full(rows, len(self.names), dtype=np.int64)])
        self.names.append(name)
        return n0, n0 + rows

    def add_to(self, ix, name):
        d = self.names.index(name)
        sel = np.flatnonzero(self.doc == d)
        ix.add(name, self.ext[sel], self.V[sel].to(DEV))

    def rows(self, ix):
        """j of every stored row, through ids_t (fails if an id is unknown or stored twice)."""
        ids = _np(ix.ids_t[:ix.n])
        assert np.array_equal(ids, ix.ids[:ix.n])
        inv = {int(e): j for j, e in enumerate(self.ext)}
        j = np.array([inv[int(e)] for e in ids], dtype=np.int64)
        assert ix.n == len(self.ext) and len(set(j.tolist())) == ix.n
        return j

    def oracle(self, ix, q, filt=None, lists=None):
        """(fp64 scores [Q, n] in row order, allowed [Q, n]): live rows of the query's documents,
        within the given probe lists (row ranges of list_off) if any."""
        j = self.rows(ix)
        S = (q.to(BF16).double().cpu() @ self.V.double().t()).numpy()[:, j]
        live = ~np.isin(self.doc[j], [self.names.index(x) for x in self.removed])
        allowed = np.tile(live, (q.shape[0], 1))
        if filt is not None:
            for qi, f in enumerate(filt):
                if f is not None:
                    allowed[qi] &= np.isin(self.doc[j], [self.names.index(x) for x in f if x in self.names])
        if lists is not None:
            for qi in range(q.shape[0]):
                inl = np.zeros(ix.n, dtype=bool)
                for l in lists[qi]:
                    if l >= 0:
                        inl[int(ix.list_off[l]):int(ix.list_off[l + 1])] = True
                allowed[qi] &= inl
        return S, allowed

    def integrity(self, ix):
        """Every external id still names the vector it was added with, under its document's slot."""
        j = self.rows(ix)
        assert torch.equal(ix.X[:ix.n].cpu().view(torch.int16), self.V[j].view(torch.int16)), "a row moved off its id"
        slot = np.array([-1 if n in self.removed else ix.docs[n].slot for n in self.names])
        assert np.array_equal(_np(ix.slots_t[:ix.n]), slot[self.doc[j]])
        lo = np.asarray(ix.list_off)
        assert lo[0] == 0 and lo[-1] == ix.trained_n and bool((np.diff(lo) >= 0).all()) and len(lo) == LISTS + 1


def _build(geom):
    dim, n = GEOMS[geom]
    co = _Corpus(dim, n)
    ix = IVFFlatIndex(dim, DEV, lists=LISTS, probes=LISTS, capacity=256, seed=1)
    for name in co.names:
        co.add_to(ix, name)
    assert ix.train(iters=4) and ix.trained_n == ix.n == n
    return ix, co


def _trained(geom):
    if geom not in _IVF:
        _IVF[geom] = _build(geom)
    return _IVF[geom]


def _queries(co, picks, seed):
    """Stored vectors (self-matches) and fresh points of the same clusters."""
    return torch.cat([co.V[picks], _clustered(3, co.dim, seed)]).to(DEV)


def _check_search(ix, co, q, k, min_sim, filt=None, lists=None):
    S, allowed = co.oracle(ix, q, filt, lists)
    return _check_rows(ix.search(q, k, min_sim, filt), S, allowed, k, thr=min_sim)


@pytest.mark.parametrize("geom", list(GEOMS))
def test_ivf_train_keeps_rows_and_assigns_the_nearest_list(geom):
    ix, co = _trained(geom)
    co.integrity(ix)
    # every row sits in the list of its best centroid, up to TOL between fp64 scores
    Sc = (ix.X[:ix.n].double() @ ix.centroids.double().t()).cpu().numpy()
    lst = np.repeat(np.arange(LISTS), np.diff(ix.list_off))
    gap = Sc.max(1) - Sc[np.arange(ix.n), lst]
    print(f"[{geom}] list sizes {np.diff(ix.list_off).tolist()}, worst assignment gap {gap.max():.3g}, "
          f"rows off their best list {(gap > 0).sum()}")
    assert float(gap.max()) <= TOL, f"{int((gap > TOL).sum())} rows are not in their nearest list (worst gap {gap.max():.3g})"


@pytest.mark.parametrize("geom", list(GEOMS))
def test_ivf_search_all_lists_is_exact(geom):
    """probes = lists: every live row is scanned (n = 6000: max_rows 6000, 12 splits)."""
    ix, co = _trained(geom)
    n = ix.n
    q = _queries(co, [0, n // 3, n - 1, int(.45 * n)], 5)
    Q = q.shape[0]
    _check_search(ix, co, q, 10, -1.0)
    _check_search(ix, co, q, 32, -1.0)
    _check_search(ix, co, q, 10, 0.75)                                   # a floor inside the clusters' scores
    filt = [["doc0"], ["doc3"], None, ["doc1", "doc4"], ["nope"], ["doc2", "doc5", "doc0"], ["doc3", "doc1"]]
    assert len(filt) == Q
    s, i = _check_search(ix, co, q, 10, -1.0, filt)
    assert int((i[1] >= 0).sum()) == 1 and not bool((i[4] >= 0).any())    # doc3 has one row; "nope" none
    _check_search(ix, co, q, 6, 0.6, filt)
    s, ids = ix.search_ids(q[:4], 1, -1.0)
    assert ids[:, 0].tolist() == co.ext[[0, n // 3, n - 1, int(.45 * n)]].tolist()   # a stored row finds itself


@pytest.mark.parametrize("geom", list(GEOMS))
def test_ivf_search_three_probes_scans_exactly_those_lists(geom):
    ix, co = _trained(geom)
    q = _queries(co, [1, ix.n // 2, ix.n - 2], 6)
    ix.probes = 3
    try:
        _, lists = ix.ops.topk_dense(ix.centroids, q.to(BF16).contiguous(), 3, -2.0)   # the index's own probe
        lists = _np(lists)
        assert lists.shape == (q.shape[0], 3) and bool((lists >= 0).all())
        _check_search(ix, co, q, 10, -1.0, lists=lists)
        _check_search(ix, co, q, 32, 0.7, [["doc2", "doc4"]] * q.shape[0], lists=lists)
    finally:
        ix.probes = LISTS


@pytest.mark.parametrize("geom", list(GEOMS))
def test_ivf_removal_delta_rows_and_retraining(geom):
    ix, co = _build(geom)
    n0 = ix.n
    assert ix.remove_doc("doc2") == int((co.doc == 2).sum())
    co.removed.add("doc2")
    q = _queries(co, [0, int(.3 * n0), n0 - 1], 7)                       # the second is a removed row
    s, i = _check_search(ix, co, q, 10, -1.0)
    _check_search(ix, co, q, 10, -1.0, [["doc2", "doc0"]] * q.shape[0])
    # delta rows, under retrain_frac: scanned exactly and merged with the lists' result
    a0, b0 = co.extend("new0", n0 // 20, 11)
    co.add_to(ix, "new0")
    a1, b1 = co.extend("new1", n0 // 25, 12)
    co.add_to(ix, "new1")
    q = torch.cat([co.V[[a0 + 7, a1 + 3, 5]].to(DEV), q])
    s, i = _check_search(ix, co, q, 10, -1.0)
    assert ix.trained_n == n0 and ix.n == b1, "retrained below retrain_frac"
    assert i[0, 0] == a0 + 7 and i[1, 0] == a1 + 3                       # delta rows keep their insertion row
    assert _np(ix.gather_ids(torch.from_numpy(i[:2, 0].copy()).to(DEV))).tolist() == co.ext[[a0 + 7, a1 + 3]].tolist()
    assert q.shape[0] == 9
    _check_search(ix, co, q, 32, 0.7, [["new0", "doc1"], ["new1"], None, ["doc5"], ["new1", "new0"], ["doc2"], None,
                                       ["doc0", "new0"], ["nope"]])
    ix.probes = 3
    _, lists = ix.ops.topk_dense(ix.centroids, q.to(BF16).contiguous(), 3, -2.0)
    lists = _np(lists)
    S, allowed = co.oracle(ix, q, None, lists)
    allowed[:, n0:] = co.oracle(ix, q)[1][:, n0:]                        # every live delta row, whatever the probes
    _check_rows(ix.search(q, 10, -1.0), S, allowed, 10, thr=-1.0)
    ix.probes = LISTS
    assert ix.remove_doc("new1") == b1 - a1
    co.removed.add("new1")
    s, i = _check_search(ix, co, q, 32, -1.0)
    assert not bool(((i >= a1) & (i < b1)).any()) and i[0, 0] == a0 + 7
    # past retrain_frac: the next search retrains and is exact over the new lists
    a2, b2 = co.extend("new2", n0 // 4 - (b1 - n0) + 10, 13)
    co.add_to(ix, "new2")
    assert ix.n - ix.trained_n > ix.retrain_frac * ix.trained_n
    q = torch.cat([co.V[[a2 + 1, a0 + 7]].to(DEV), q[3:]])
    got = ix.search(q, 10, -1.0)
    assert ix.trained_n == ix.n == b2
    co.integrity(ix)
    S, allowed = co.oracle(ix, q)
    _check_rows(got, S, allowed, 10, thr=-1.0)
    s, ids = ix.search_ids(q[:2], 1, -1.0)
    assert ids[:, 0].tolist() == co.ext[[a2 + 1, a0 + 7]].tolist()
    assert q.shape[0] == 8
    _check_search(ix, co, q, 10, 0.7, [["new2", "new1"], ["new0"], None, ["doc2"], ["doc4", "new2"], ["new1"], None,
                                       ["doc0"]])


def test_ivf_needs_dim_multiple_of_32():
    """dim 72 (% 8, not % 32) cannot run as an IVF index on the GPU: the centroid scans go through
    topk_dense, which takes d % 32 == 0 only. It says so instead of computing something else."""
    ix = IVFFlatIndex(72, DEV, lists=4)
    ix.add("a", np.arange(64), _clustered(64, 72, 1).to(DEV))
    with pytest.raises(ValueError, match="d % 32"):
        ix.train(iters=1)


# --------------------------------------------------------------------- duplicate documents in a filter
@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_flat_filter_naming_a_document_twice(dtype):
    """The narrow (range scan) path: a document named twice is scanned once."""
    d, k = 768, 10
    x = _unit(2000, d, 3)
    ix = FlatIndex(d, DEV, dtype=dtype)
    for name, (a, b) in {"A": (0, 100), "B": (100, 250), "C": (250, 1900)}.items():
        ix.add(name, np.arange(a, b), x[a:b].to(DEV))
    ix.add("A", np.arange(1900, 2000), x[1900:].to(DEV))                 # A has two ranges
    q = x[[1950]].to(DEV)
    for dup, plain in (([["A", "A"]], [["A"]]), ([["A", "B", "A"]], [["A", "B"]])):
        assert ix._ranges_for(dup)[2] * 1 <= 4 * ix.n                    # the narrow path's condition
        s, i = ix.search(q, k, -1.0, dup)
        s0, i0 = ix.search(q, k, -1.0, plain)
        live = i[0][i[0] >= 0].tolist()
        assert len(live) == k and len(set(live)) == k, f"a row came back twice: {i[0].tolist()}"
        assert live[0] == 1950
        assert torch.equal(i, i0) and torch.equal(s, s0)
