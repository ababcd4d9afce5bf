"""fp8 (e4m3) flat vector index kernels (csrc/vecsearch8.hip) against the reference.

Tolerance of the scans, derived: the kernels and the fp32 reference add the same d <= 1024 exact
products code_i * scale * q_i in different orders; with sum |x_i q_i| <= 1 (unit rows and queries)
two fp32 summation orders differ by at most d * 2^-24 ~ 6.1e-5, so
  * a returned score is within TOL = 1e-4 of the reference's score at that rank,
  * a returned id's reference score is within TOL of the returned score,
  * a returned id's reference score is no more than TOL below the reference's k-th score
(ids themselves may differ between rows whose scores are closer than that).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from docagents_amd.index.flat import FlatIndex  # noqa: E402
from docagents_amd.ops import kernels as K  # noqa: E402
from docagents_amd.ops import reference as R  # noqa: E402

from kernel_frames import assert_frame_intact, fill_pattern  # noqa: E402

DEV = "cuda"
BF16 = torch.bfloat16
TOL = 1e-4


def _unit(n, d, seed, device=DEV):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=-1).to(device)


def _quant(X):
    """codes uint8 [N, d] / scale fp32 [N] of bf16 rows (reference quantiser, on the rows' device)."""
    q, s = R.quant_weight_fp8_pow2(X)
    return q.view(torch.uint8).contiguous(), s.contiguous()


def _check(got, full, valid, Kk):
    """The 1e-4 rule. full [Q, N]: the reference's fp32 scores of every row; valid [Q, N]: the rows a
    query may return (filter, floor within TOL handled by the caller through ``full``)."""
    s, i = got[0].cpu(), got[1].cpu().long()
    full, valid = full.cpu(), valid.cpu()
    ref = full.masked_fill(~valid, float("-inf"))
    rs = torch.sort(ref, dim=1, descending=True).values[:, :Kk]
    if rs.shape[1] < Kk:
        rs = torch.cat([rs, torch.full((rs.shape[0], Kk - rs.shape[1]), float("-inf"))], 1)
    live = i >= 0
    assert bool((s[~live] == float("-inf")).all())
    assert torch.equal(live.sum(1), torch.isfinite(rs).sum(1)), "fewer / more rows than the reference returns"
    # scores per rank (a rank the reference fills is filled, unless its score sits within TOL of the floor)
    both = live & torch.isfinite(rs)
    assert float((s - rs)[both].abs().max() if both.any() else 0.0) <= TOL, float((s - rs)[both].abs().max())
    own = torch.gather(full, 1, i.clamp_min(0))
    assert float((own - s)[live].abs().max() if live.any() else 0.0) <= TOL
    kth = rs[:, -1:].expand_as(own)
    assert bool((own[live] >= kth[live] - TOL).all())
    assert bool(torch.gather(valid, 1, i.clamp_min(0))[live].all()), "a row outside the filter came back"
    for q in range(i.shape[0]):  # no row twice
        r = i[q][live[q]].tolist()
        assert len(set(r)) == len(r)
    return s, i


# ------------------------------------------------------------------------------------------ quantiser
@pytest.mark.parametrize("n", [1, 17, 300])
@pytest.mark.parametrize("d", [128, 384, 768, 1024])
def test_index_quant_rows(n, d):
    g = torch.Generator().manual_seed(n * d)
    X = (_unit(n, d, n + d) * (0.05 + 2.0 * torch.rand(n, 1, generator=g).to(DEV))).to(BF16)
    X[n // 2] = 0.0                                     # all-zero row (n = 1: the only one)
    if n > 1:
        X[n - 1] *= 0.1
        X[n - 1, 3] = -448.0 * 2.0 ** -10               # amax exactly on a 448 * 2^e boundary
        X[0] *= 0.1
        X[0, 5] = 1.7578125 * 2.0 ** -2                 # one bf16 step above 1.75 * 2^E: the next exponent
    X = X.contiguous()
    row0, cap = 5, n + 5 + 9
    codes = fill_pattern(torch.empty((cap, d), dtype=torch.uint8, device=DEV))
    scale = fill_pattern(torch.empty(cap, dtype=torch.float32, device=DEV))
    K.index_quant_rows(X, codes, scale, row0)
    torch.cuda.synchronize()
    q, s = R.quant_weight_fp8_pow2(X)
    assert torch.equal(codes[row0:row0 + n], q.view(torch.uint8))
    assert torch.equal(scale[row0:row0 + n], s)
    assert float(scale[row0 + n // 2]) == 1.0 and not bool(codes[row0 + n // 2].any())
    if n > 1:
        assert float(scale[row0 + n - 1]) == 2.0 ** -10 and int(codes[row0 + n - 1, 3]) == 0xFE
        assert float(scale[row0]) == 2.0 ** -9
    assert_frame_intact(codes, (slice(row0, row0 + n), slice(0, d)), "codes")
    assert_frame_intact(scale, (slice(row0, row0 + n),), "scale")


# ------------------------------------------------------------------------------------------ dense scan
_DENSE = {}


def _dense_case(N, d, Q):
    """Rows, queries, codes and the fp32 scores of every (query, dequantised row): computed once per shape."""
    key = (N, d, Q)
    if key not in _DENSE:
        X = _unit(N, d, N).to(BF16)
        Qv = _unit(Q, d, N + 1).to(BF16)
        Qv[0] = X[N // 2]
        codes, scale = _quant(X)
        full = Qv.float() @ R.index_dequant(codes, scale).float().t()
        _DENSE[key] = (codes, scale, Qv.contiguous(), full)
    return _DENSE[key]


SHAPES = [(63, 768, 1, 3), (1000, 768, 5, 5), (3000, 128, 16, 5), (7000, 384, 3, 32), (2000, 768, 17, 3),
          (5000, 1024, 37, 20), (3000, 768, 300, 4)]


@pytest.mark.parametrize("mode", ["plain", "filter_floor", "removed"])
@pytest.mark.parametrize("N,d,Q,Kk", SHAPES)
def test_topk_dense8(N, d, Q, Kk, mode):
    """The fp8 streaming scan (<= 16 queries), the shared-tile scan (17+; 300 = two passes of the
    256-query limit, five query groups) vs fp32 over the dequantised rows: plain, filtered + floored,
    and with removed rows (slot -1)."""
    codes, scale, Qv, full = _dense_case(N, d, Q)
    everything = torch.ones_like(full, dtype=torch.bool)
    if mode == "plain":
        s, i = _check(K.topk_dense8(codes, scale, Qv, Kk, -1.0), full, everything, Kk)
        assert int(i[0, 0]) == N // 2
        return
    if mode == "filter_floor":
        slots = (torch.arange(N, device=DEV, dtype=torch.int32) // 10).contiguous()
        W = (N // 10 + 32) // 32
        bitmap = torch.zeros(Q, W, dtype=torch.int32, device=DEV)
        bitmap[:, 0] = 0b1011
        bitmap[0, (N // 2 // 10) >> 5] |= (1 << ((N // 2 // 10) & 31))
        thr = 0.0
        got = K.topk_dense8(codes, scale, Qv, Kk, thr, slots=slots, bitmap=bitmap)
        sl = slots.long()
        bits = ((bitmap[:, sl >> 5] >> (sl & 31).view(1, -1)) & 1).bool()
        # rows whose reference score is within TOL of the floor may fall on either side of it: they may
        # come back (valid) but do not have to (not counted by the reference ranks)
        s, i = got[0].cpu(), got[1].cpu().long()
        near = (full - thr).abs() <= TOL
        must = bits & (full >= thr) & ~near
        may = bits & ((full >= thr) | near)
        returned = torch.zeros_like(full, dtype=torch.bool).cpu()
        returned.scatter_(1, i.clamp_min(0), i >= 0)
        valid = must | (may & returned.to(may.device))
        _check(got, full, valid, Kk)
        assert bool((s[i >= 0] >= thr).all())
        assert int(i[0, 0]) == N // 2
        return
    slots2 = torch.zeros(N, dtype=torch.int32, device=DEV)
    slots2[N // 2] = -1
    slots2[::7] = -1
    s, i = _check(K.topk_dense8(codes, scale, Qv, Kk, -1.0, slots=slots2), full,
                  everything & (slots2 >= 0).view(1, -1), Kk)
    assert not bool((i == N // 2).any()) and not bool(((i >= 0) & (i % 7 == 0)).any())


@pytest.mark.parametrize("Q", [3, 20, 64])
def test_topk_dense8_ties(Q):
    """Exact score ties at the k-th place go to the smaller row id: 50 copies of one row (identical
    codes and scales, so bit-identical scores) plus ten more in another row block, queried with that
    row, must return the 8 smallest ids."""
    N, d, Kk = 20000, 1024, 8
    X = _unit(N, d, Q).to(BF16)
    X[7000:7050] = X[7000]
    X[150:160] = X[7000]
    Qv = _unit(Q, d, Q + 100).to(BF16)
    Qv[Q - 1] = X[7000]
    codes, scale = _quant(X)
    s, i = K.topk_dense8(codes, scale, Qv.contiguous(), Kk, -1.0)
    assert i[Q - 1].tolist() == list(range(150, 158))
    assert bool((s[Q - 1] == s[Q - 1, 0]).all())
    full = Qv.float() @ R.index_dequant(codes, scale).float().t()
    _check((s, i), full, torch.ones_like(full, dtype=torch.bool), Kk)


def test_topk_dense8_rejects_what_it_does_not_take():
    X = _unit(100, 256, 1).to(BF16)
    codes, scale = _quant(X)
    with pytest.raises(ValueError, match="fp8 dense scan"):
        K.topk_dense8(codes, scale, X[:2].contiguous(), 3, -1.0)
    with pytest.raises(ValueError, match="fp8 index"):
        FlatIndex(256, DEV, dtype="fp8")


# ------------------------------------------------------------------------------------------ ranges scan
def test_topk_ranges8():
    N, d, Q, Kk = 3000, 768, 4, 6
    X = _unit(N, d, 1).to(BF16)
    Qv = _unit(Q, d, 2).to(BF16).contiguous()
    codes, scale = _quant(X)
    rg = [[0, 10], [100, 700], [2990, 3000], [5, 6], [0, 3000], [1000, 1001]]
    ro = [0, 3, 4, 5, 6]
    ranges = torch.tensor(rg, dtype=torch.int32, device=DEV)
    roff = torch.tensor(ro, dtype=torch.int32, device=DEV)
    full = Qv.float() @ R.index_dequant(codes, scale).float().t()
    allowed = torch.zeros_like(full, dtype=torch.bool)
    for q in range(Q):
        for a, b in rg[ro[q]:ro[q + 1]]:
            allowed[q, a:b] = True
    for rps in (256, 512):
        got = K.topk_ranges8(codes, scale, Qv, ranges, roff, Kk, -1.0, max_rows=3000, rows_per_split=rps)
        s, i = _check(got, full, allowed, Kk)
        assert int(i[1, 0]) == 5 and int(i[1, 1]) == -1  # single-row range
    # removed rows and a floor
    slots = torch.zeros(N, dtype=torch.int32, device=DEV)
    slots[::3] = -1
    got = K.topk_ranges8(codes, scale, Qv, ranges, roff, Kk, -1.0, max_rows=3000, slots=slots)
    s, i = _check(got, full, allowed & (slots >= 0).view(1, -1), Kk)
    assert not bool(((i >= 0) & (i % 3 == 0)).any())


# ------------------------------------------------------------------------------------------ the index
def _drive(ix, x):
    ix.add("d0", np.arange(300), x[:300])
    ix.add("d1", np.arange(300, 1000), x[300:1000])                       # grows past the capacity
    ix.add_bulk(["d2", "d3", "d4"], [800, 700, 400], np.arange(1000, 2900), x[1000:2900])
    ix.add("d0", np.arange(2900, 3000), x[2900:3000])
    ix.remove_doc("d3")
    ix.remove_keys("d2", [1005, 1006, 1500, 1799])
    ix.remove_keys("d0", [0, 2999])


def test_flat_index_fp8_gpu_matches_cpu():
    """3000 x 768 through adds, growth and removals: identical codes on both devices, and every
    search path (dense, ranges, bitmap) of the GPU index against the CPU index under the 1e-4 rule."""
    d = 768
    x = _unit(3000, d, 11, "cpu")
    g, c = FlatIndex(d, DEV, capacity=512, dtype="fp8"), FlatIndex(d, "cpu", capacity=512, dtype="fp8")
    _drive(g, x.to(DEV))
    _drive(c, x)
    assert g.n == c.n == 3000 and g.nbytes() == 3000 * (d + 4)
    assert torch.equal(g.codes[:g.n].cpu(), c.codes[:c.n]) and torch.equal(g.scale[:g.n].cpu(), c.scale[:c.n])
    assert torch.equal(g.slots_t[:g.n].cpu(), c.slots_t[:c.n])
    assert torch.equal(g.state_dict()["X"], c.state_dict()["X"])
    q = torch.cat([x[[3, 400, 1200, 2000, 2950]], _unit(3, d, 12, "cpu")]).to(BF16)
    Q = q.shape[0]
    full = q.float() @ R.index_dequant(c.codes[:c.n], c.scale).float().t()
    live = (c.slots_t[:c.n] >= 0).view(1, -1)
    every = [f"d{i}" for i in range(5)]

    def allowed(filt):
        m = torch.zeros(Q, c.n, dtype=torch.bool)
        for qi, f in enumerate(filt):
            for doc in (c.docs if f is None else f):
                for a, b in (c.docs[doc].ranges if doc in c.docs else []):
                    m[qi, a:b] = True
        return m

    cases = [(10, -1.0, None), (5, 0.05, None), (10, -1.0, [["d4"]] * Q),
             (8, -1.0, [["d0"], ["d2"], ["d3"], None, ["d1", "d4"], ["nope"], ["d2", "d0"], ["d4"]]),
             (10, -1.0, [every] * Q), (32, 0.02, [every[:3]] * Q)]
    for k, thr, filt in cases:
        got = g.search(q.to(DEV), k, thr, filt)
        valid = (live.expand(Q, -1) if filt is None else allowed(filt) & live)
        near = (full - thr).abs() <= TOL
        i = got[1].cpu().long()
        returned = torch.zeros_like(full, dtype=torch.bool).scatter_(1, i.clamp_min(0), i >= 0)
        valid = valid & (((full >= thr) & ~near) | (near & returned))
        _check(got, full, valid, k)
    s, ids = g.search_ids(q[:5].to(DEV), 1, -1.0)
    assert ids[[0, 1, 2, 4], 0].tolist() == [3, 400, 1200, 2950]  # a live row finds itself
    assert 2000 not in g.search_ids(q[3:4].to(DEV), 32, -1.0)[1][0].tolist()  # d3 was removed


@pytest.mark.parametrize("scenario", ["test_search_sees_the_whole_add_or_nothing",
                                      "test_search_never_returns_removed_rows"])
def test_fp8_index_writes_against_concurrent_searches(scenario, monkeypatch):
    """tests/test_index_race_gpu.py's two scenarios on an fp8 flat index: the quantising add (and its
    growth) or the slot masking is still pending on the writer's stream when another stream searches."""
    import test_index_race_gpu as race
    made = []

    def mk(kind, dev, d):
        made.append(FlatIndex(d, dev, capacity=64, dtype="fp8"))
        return made[-1]
    monkeypatch.setattr(race, "_mk", mk)
    getattr(race, scenario)("flat")
    assert len(made) == 1 and made[0].dtype == "fp8" and made[0].n > 64


def test_engine_with_fp8_index_on_the_gpu():
    from test_index8_cpu import engine_smoke
    eng = engine_smoke("cuda", TOL)
    assert eng.index.codes.is_cuda
