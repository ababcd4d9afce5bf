"""The fp8 (e4m3) IVFFlat index on the GPU (INDEX_KIND=ivfflat_fp8): the k-means update over codes, the
row dequantiser, the scattering quantiser, and the index itself, each against an exact oracle.

Oracles of the index: fp64 scores of the DEQUANTISED STORED rows (``codes * scale``, exact in bf16),
restricted to live rows, the filter and the probed lists. An fp8 index is the bf16 index over that matrix.

Tolerance of a score, TOL8 = 1e-4: the bound tests/test_index8_gpu.py uses for the fp8 scans. The range
scan adds d <= 1024 exact products in fp32 and applies the power-of-two scale exactly; with unit rows
and queries that is at most d * 2^-24 <= 6.1e-5 from the exact sum. A row within TOL8 of a similarity
floor may fall on either side of it.
Largest |returned score - fp64 score| over every case of this file on an MI355X: 8.75e-8.

Nearest list: every row sits in the list of its best centroid up to 2 * d * 2^-24 between fp64 scores
(two fp32 sums of d exact products, sum |x_i c_i| <= ||x|| ||c|| ~ 1): 9.2e-5 at d = 768, 1.5e-5 at 128.
Worst gap measured on an MI355X: 0 at both geometries (no row off its best list).

kmeans_accum8: the summation bound of tests/test_ivf_gpu.py::_accum_check, unchanged: the terms
(an e4m3 value times a power of two) are exact in fp32.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from docagents_amd.index.flat import _pad4  # noqa: E402
from docagents_amd.index.ivf import IVFFlatIndex  # noqa: E402
from docagents_amd.index.snapshot import load_index, save_index  # noqa: E402
from docagents_amd.ops import kernels as K  # noqa: E402
from docagents_amd.ops import reference as R  # noqa: E402

from test_ivf_gpu import U, _assert_topk, _clustered, _Corpus, _floored, _np  # noqa: E402

DEV = "cuda"
BF16 = torch.bfloat16
TOL8 = 1e-4
MAX_ERR = [0.0]


def _quant(x):
    """(codes uint8, scale fp32) of bf16 rows by the host reference."""
    q, s = R.quant_weight_fp8_pow2(x.to(BF16))
    return q.view(torch.uint8).contiguous(), s.contiguous()


# ----------------------------------------------------------------------------------------- kmeans_accum8
def _accum8_check(codes, scale, Xd, assign, s0, c0):
    """tests/test_ivf_gpu.py::_accum_check for the fp8 kernel, against fp64 sums of the dequantised rows."""
    L, d = s0.shape
    sums, counts = s0.clone(), c0.clone()
    K.kmeans_accum8(codes, scale, assign, sums, counts)
    torch.cuda.synchronize()
    a = assign.long()
    m = a >= 0
    n_c = torch.bincount(a[m], minlength=L)
    assert torch.equal(counts, c0 + n_c.float()), "counts"
    exact, absum = s0.double(), s0.double().abs()
    exact.index_add_(0, a[m], Xd[m])
    absum.index_add_(0, a[m], Xd[m].abs())
    terms = n_c.double()[:, None] + (s0 != 0).double()
    adds = (terms - 1).clamp_min(0)
    bound = adds * U * absum / (1 - adds * U) + terms * 2.0 ** -53 * absum
    over = (sums.double() - exact).abs() - bound
    print(f"kmeans_accum8: worst (error - bound) {float(over.max()):.3g}, worst error "
          f"{float((sums.double() - exact).abs().max()):.3g}")
    assert float(over.max()) <= 0, f"sum error {float(over.max()):.3g} above the summation bound"
    idle = n_c == 0
    assert torch.equal(sums.view(torch.int32)[idle], s0.view(torch.int32)[idle]), "a list that got no row changed"
    return n_c


@pytest.mark.parametrize("L", [1, 10, 300])
@pytest.mark.parametrize("N,d", [(1, 16), (700, 112), (5000, 768), (3000, 1024)])
def test_kmeans_accum8_exact(N, d, L):
    g = torch.Generator().manual_seed(N + d + L)
    X = torch.randn(N, d, generator=g).to(BF16)
    if N > 4:
        X[3] = 0.0                                          # an all-zero row: scale 1, adds zeros
    codes, scale = _quant(X)
    keep_c, keep_s = codes.clone(), scale.clone()
    Xd = R.index_dequant(codes, scale).double().to(DEV)
    codes, scale = codes.to(DEV), scale.to(DEV)
    zero_s, zero_c = torch.zeros(L, d, device=DEV), torch.zeros(L, device=DEV)
    # onto non-zero sums and counts (with a -0.0 and a denormal that only survive untouched)
    s0 = torch.randn(L, d, generator=g).to(DEV)
    s0[L - 1, 0], s0[L - 1, d - 1] = -0.0, 1e-41
    c0 = torch.randint(0, 9, (L,), generator=g).float().to(DEV)
    assign = torch.randint(-1, L, (N,), generator=g, dtype=torch.int32).to(DEV)
    if N > 1:
        assign[assign == L - 1] = -1                        # list L - 1 gets no row (L = 1: no row at all)
    n_c = _accum8_check(codes, scale, Xd, assign, s0, c0)
    assert N == 1 or int(n_c[L - 1]) == 0
    # every row into one list: every atomic of a column lands on one address
    n_c = _accum8_check(codes, scale, Xd, torch.full((N,), L - 1, dtype=torch.int32, device=DEV), zero_s, zero_c)
    assert int(n_c[L - 1]) == N
    # nothing assigned: nothing changes
    sums, counts = s0.clone(), c0.clone()
    K.kmeans_accum8(codes, scale, torch.full((N,), -1, dtype=torch.int32, device=DEV), sums, counts)
    torch.cuda.synchronize()
    assert torch.equal(sums.view(torch.int32), s0.view(torch.int32)) and torch.equal(counts, c0)
    assert torch.equal(codes.cpu(), keep_c) and torch.equal(scale.cpu(), keep_s), "the rows were written to"
    with pytest.raises(ValueError):
        K.kmeans_accum8(codes, scale, assign[:-1] if N > 1 else assign.long(), sums, counts)


# ------------------------------------------------------------- index_dequant_rows, index_quant_rows(dest=)
@pytest.mark.parametrize("n", [1, 63, 1000])
@pytest.mark.parametrize("d", [16, 128, 768, 1024])
def test_dequant_rows_and_quant_scatter_are_bit_exact_and_write_nothing_else(d, n):
    g = torch.Generator().manual_seed(d + n)
    cap = n + 37
    X = torch.randn(cap, d, generator=g).to(BF16) * torch.exp2(torch.randint(-12, 4, (cap, 1), generator=g).float()).to(BF16)
    X[cap // 2] = 0.0
    codes_h, scale_h = _quant(X)
    deq = R.index_dequant(codes_h, scale_h)
    codes = codes_h.to(DEV)
    scale = torch.ones(_pad4(cap), device=DEV)
    scale[:cap] = scale_h.to(DEV)
    keep_c, keep_s = codes.clone(), scale.clone()
    sent = torch.tensor(-7.25, dtype=BF16)

    def dequant(**kw):
        big = torch.full((n + 2, d), float(sent), dtype=BF16, device=DEV)
        out = K.index_dequant_rows(codes, scale, big[1:n + 1], **kw)
        torch.cuda.synchronize()
        assert out.data_ptr() == big[1].data_ptr()
        assert bool((big[0] == sent).all()) and bool((big[n + 1] == sent).all()), "wrote outside out"
        assert torch.equal(codes, keep_c) and torch.equal(scale, keep_s), "the store was written to"
        return big[1:n + 1].cpu()

    assert torch.equal(dequant().view(torch.int16), deq[:n].view(torch.int16))
    assert torch.equal(dequant(row0=37).view(torch.int16), deq[37:37 + n].view(torch.int16))
    sel = torch.randint(0, cap, (n,), generator=g)
    if n > 2:
        sel[1] = sel[0]                                     # repeats
        sel[n - 1] = cap - 1
    assert torch.equal(dequant(sel=sel.to(DEV)).view(torch.int16), deq[sel].view(torch.int16))
    with pytest.raises(ValueError):
        K.index_dequant_rows(codes, scale, torch.empty((n, d), dtype=BF16, device=DEV), row0=38)
    bad = sel.clone()
    bad[0] = cap
    with pytest.raises(ValueError):
        K.index_dequant_rows(codes, scale, torch.empty((n, d), dtype=BF16, device=DEV), sel=bad.to(DEV))

    # the scatter: a random permutation into a larger store filled with sentinels
    big_c = torch.full((cap, d), 0xAB, dtype=torch.uint8, device=DEV)
    big_s = torch.full((_pad4(cap),), 7.0, device=DEV)
    dest = torch.randperm(cap, generator=g)[:n]
    rows = X[:n].to(DEV).contiguous()
    K.index_quant_rows(rows, big_c, big_s, dest=dest.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(big_c.cpu()[dest], codes_h[:n]) and torch.equal(big_s.cpu()[dest], scale_h[:n])
    rest = torch.ones(_pad4(cap), dtype=torch.bool)
    rest[dest] = False
    assert bool((big_c.cpu()[rest[:cap]] == 0xAB).all()) and bool((big_s.cpu()[rest] == 7.0).all()), \
        "a byte outside the named rows changed"
    assert torch.equal(rows.cpu().view(torch.int16), X[:n].view(torch.int16))
    bad = dest.clone()
    bad[n - 1] = cap
    with pytest.raises(ValueError):
        K.index_quant_rows(rows, big_c, big_s, dest=bad.to(DEV))
    with pytest.raises(ValueError):
        K.index_quant_rows(rows, big_c, big_s, 1, dest=dest.to(DEV))


# ------------------------------------------------------------------------------------------------- IVF
# dim 768, n 6000: the GEMM + argmax assignment with the exact re-check (n >= 4096, dim % 64 == 0) over
# dequantised slices, and 12 scan splits; dim 128, n 2000: the topk_dense assignment.
GEOMS = {"gemm768": (768, 6000), "dense128": (128, 2000)}
LISTS = 16
_IVF = {}


def _deq_rows(ix):
    return R.index_dequant(ix.codes[:ix.n].cpu(), ix.scale[:ix.n].cpu())


class _Corpus8(_Corpus):
    def oracle(self, ix, q, filt=None, lists=None):
        """As _Corpus.oracle, the scores those of the dequantised stored rows."""
        _, allowed = super().oracle(ix, q, filt, lists)
        S = (q.to(BF16).double().cpu() @ _deq_rows(ix).double().t()).numpy()
        return S, allowed

    def integrity(self, ix, lists=LISTS):
        """Every external id still names quant_weight_fp8_pow2 of the vector it was added with (codes and
        scale bit for bit), under its document's slot; list_off is monotone and ends at trained_n."""
        j = self.rows(ix)
        codes, scale = _quant(self.V[j])
        assert torch.equal(ix.codes[:ix.n].cpu(), codes), "a row's codes moved off its id"
        assert torch.equal(ix.scale[:ix.n].cpu(), scale), "a row's scale moved off its id"
        assert ix.scale.numel() == _pad4(ix.codes.shape[0]) and bool((ix.scale[ix.n:] == 1).all()), "scale tail"
        assert ix.scale.data_ptr() % 16 == 0 and ix.codes.data_ptr() % 16 == 0
        slot = np.array([-1 if n in self.removed else ix.docs[n].slot for n in self.names])
        assert np.array_equal(_np(ix.slots_t[:ix.n]), slot[self.doc[j]])
        lo = np.asarray(ix.list_off)
        assert lo[0] == 0 and lo[-1] == ix.trained_n and bool((np.diff(lo) >= 0).all()) and len(lo) == lists + 1


def _build(geom):
    dim, n = GEOMS[geom]
    co = _Corpus8(dim, n)
    ix = IVFFlatIndex(dim, DEV, lists=LISTS, probes=LISTS, capacity=256, seed=1, dtype="fp8")
    for name in co.names:
        co.add_to(ix, name)
    assert ix.train(iters=4) and ix.trained_n == ix.n == n
    assert ix.dtype == "fp8" and not hasattr(ix, "X")
    return ix, co


def _trained(geom):
    if geom not in _IVF:
        _IVF[geom] = _build(geom)
    return _IVF[geom]


def _queries(co, picks, seed):
    return torch.cat([co.V[picks], _clustered(3, co.dim, seed)]).to(DEV)


def _check_rows(got, S, allowed, Kk, thr=None):
    s, i = _np(got[0]), _np(got[1])
    assert s.shape == (S.shape[0], Kk) and s.dtype == np.float32 and i.dtype == np.int32
    for q in range(S.shape[0]):
        al = allowed[q] if thr is None else _floored(S[q], allowed[q], thr, i[q], TOL8)
        _assert_topk(s[q], i[q], S[q], al, Kk, TOL8)
        real = i[q] >= 0
        MAX_ERR[0] = max(MAX_ERR[0], float(np.abs(s[q][real] - S[q][i[q][real]]).max(initial=0.0)))
        if thr is not None:
            assert bool((s[q][real] >= thr).all())
    print(f"largest |score - fp64| so far {MAX_ERR[0]:.3g}")
    return s, i


def _check_search(ix, co, q, k, min_sim, filt=None, lists=None):
    S, allowed = co.oracle(ix, q, filt, lists)
    return _check_rows(ix.search(q, k, min_sim, filt), S, allowed, k, thr=min_sim)


@pytest.mark.parametrize("geom", list(GEOMS))
def test_ivf8_train_keeps_rows_and_assigns_the_nearest_list(geom):
    ix, co = _trained(geom)
    co.integrity(ix)
    Sc = (_deq_rows(ix).double() @ ix.centroids.double().cpu().t()).numpy()
    lst = np.repeat(np.arange(LISTS), np.diff(ix.list_off))
    gap = Sc.max(1) - Sc[np.arange(ix.n), lst]
    bound = 2 * ix.dim * 2.0 ** -24
    print(f"[{geom}] list sizes {np.diff(ix.list_off).tolist()}, worst assignment gap {gap.max():.3g} "
          f"(bound {bound:.3g}), rows off their best list {(gap > 0).sum()}")
    assert float(gap.max()) <= bound, f"{int((gap > bound).sum())} rows are not in their nearest list (worst gap {gap.max():.3g})"


@pytest.mark.parametrize("geom", list(GEOMS))
def test_ivf8_search_all_lists_is_exact(geom):
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
def test_ivf8_search_three_probes_scans_exactly_those_lists(geom):
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
def test_ivf8_removal_delta_rows_and_retraining(geom):
    ix, co = _build(geom)
    n0 = ix.n
    assert ix.remove_doc("doc2") == int((co.doc == 2).sum())
    co.removed.add("doc2")
    q = _queries(co, [0, int(.3 * n0), n0 - 1], 7)                       # the second is a removed row
    _check_search(ix, co, q, 10, -1.0)
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
    # remove_keys: list-major rows leave search through their slot, and come back as delta rows
    assert ix.remove_keys("doc0", co.ext[[1, 2]]) == 2
    s, ids = ix.search_ids(co.V[[1, 2, 3]].to(DEV), 1, -1.0)
    assert int(ids[2, 0]) == int(co.ext[3]) and not bool(np.isin(_np(ids[:2, 0]), co.ext[[1, 2]]).any())
    ix.add("doc0", co.ext[[1, 2]], co.V[[1, 2]].to(DEV))
    s, ids = ix.search_ids(co.V[[1, 2]].to(DEV), 1, -1.0)
    assert ids[:, 0].tolist() == co.ext[[1, 2]].tolist() and ix.n == b2 + 2 and ix.trained_n == b2


def test_ivf8_build_streaming():
    """dim 128, 3 chunks of 1500 / 1500 / 700 rows, lists = 8: every chunk quantised straight into its
    destination rows of an exactly sized store."""
    dim, n, chunk, per_doc, base, lists = 128, 3700, 1500, 37, 900, 8
    X = _clustered(n, dim, 77)
    Xg = X.to(DEV)
    keep = Xg.clone()
    torch.manual_seed(3)
    ix = IVFFlatIndex(dim, DEV, lists=lists, probes=lists, seed=2, dtype="fp8")
    ix.build_streaming(lambda c: Xg[c * chunk:(c + 1) * chunk], n, chunk, per_doc, iters=4, sample=1024, id_base=base)
    assert torch.equal(Xg.view(torch.int16), keep.view(torch.int16)), "the generator's rows were written to"
    assert ix.n == ix.trained_n == n and ix.codes.shape == (n, dim) and ix.scale.numel() == _pad4(n)
    co = _Corpus8.__new__(_Corpus8)
    co.dim, co.V, co.ext = dim, X, base + np.arange(n, dtype=np.int64)
    co.doc = np.arange(n) // per_doc
    co.names = [f"d{i}" for i in range((n + per_doc - 1) // per_doc)]
    co.removed = set()
    co.integrity(ix, lists)
    q = torch.cat([Xg[[0, 1700, n - 1]], _clustered(2, dim, 78).to(DEV)])
    _check_search(ix, co, q, 10, -1.0)
    _check_search(ix, co, q, 32, 0.7, [["d0"], ["d45", "d46"], None, ["d100"], ["nope"]])
    s, ids = ix.search_ids(q[:3], 1, -1.0)
    assert ids[:, 0].tolist() == [base, base + 1700, base + n - 1]


def test_ivf8_snapshot_round_trip(tmp_path):
    ix, co = _trained("gemm768")
    path = save_index(ix, str(tmp_path / "ivf8.safetensors"), durable=False)
    b = IVFFlatIndex(ix.dim, DEV, lists=LISTS, probes=LISTS, seed=1, dtype="fp8")
    assert load_index(b, path) == ix.n and b.trained_n == ix.n
    assert torch.equal(b.centroids.view(torch.int16), ix.centroids.view(torch.int16))
    co.integrity(b)                                                       # the saved codes, bit for bit, by id
    src = {int(e): r for r, e in enumerate(ix.ids[:ix.n])}
    r = np.array([src[int(e)] for e in b.ids[:b.n]])
    assert torch.equal(b.codes[:b.n].cpu(), ix.codes[:ix.n].cpu()[r]) and torch.equal(b.scale[:b.n].cpu(), ix.scale[:ix.n].cpu()[r])
    q = _queries(co, [0, ix.n // 2, ix.n - 1], 9)
    for filt in (None, [["doc0"], ["doc3"], None, ["doc1", "doc4"], ["nope"], ["doc5"]]):
        sa, ia = ix.search_ids(q, 10, 0.3, filt)
        sb, ib = b.search_ids(q, 10, 0.3, filt)
        assert torch.equal(ia, ib), "the loaded index returns other rows"
        assert float((sa - sb).abs().nan_to_num(0.0).max()) <= 2 * TOL8
        _check_search(b, co, q, 10, 0.3, filt)
