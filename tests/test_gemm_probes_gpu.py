"""Every GEMM entry point of ops/kernels.py on the exact-integer operands of tests/gemm_probes.py: the
output must equal the fp64 reference bit for bit (a rounded element: either neighbour), so one
dropped, doubled or mispaired term of one output fails. Each test asserts the planned family and
tile (ops/gemm_plan.py), so a shape cannot silently move to another kernel; the fp8-weight ops run on
the same W as their bf16 sibling and meet the same criterion, not just the sibling's bits.

Shapes: the smallest that reach each route's edges (one row block and one more, ragged M / N, one
k-tile, K that is no multiple of the prefetch depth, every split count the planner uses). A few
cases per route run with row-padded a / out / resid (the padding holds 3.0: a stray read shows)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from docagents_amd.ops import gemm_plan as P  # noqa: E402
from docagents_amd.ops import kernels as K  # noqa: E402
from docagents_amd.ops import reference as R  # noqa: E402

import gemm_probes as G  # noqa: E402
from attn_probes import rope_table_90  # noqa: E402
from gemm_probes import EPI_BIAS, EPI_GELU, EPI_NONE, EPI_RESID, EPI_SWIGLU  # noqa: E402

DEV = "cuda"
BF16, F16 = torch.bfloat16, torch.float16
DECODE_EPIS = (EPI_NONE, EPI_BIAS, EPI_RESID, EPI_SWIGLU)
ALL_EPIS = (EPI_NONE, EPI_BIAS, EPI_GELU, EPI_RESID, EPI_SWIGLU)


class _Ops:
    """A GemmCase and its device operands."""

    def __init__(self, M, N, Kd, dtype=BF16, fp8_act=False):
        self.case = c = G.GemmCase(M, N, Kd, fp8_act=fp8_act)
        self.dtype = dtype
        self.w = c.w.to(dtype).to(DEV)
        self.bias = c.bias.to(dtype).to(DEV)
        self.resid = c.resid.to(dtype).to(DEV)
        assert torch.equal(self.resid.float().cpu(), c.resid)
        self.sa = None if c.sa is None else c.sa.to(DEV)
        self._a, self._w8 = {}, None

    def a(self, l):
        if l not in self._a:
            t = self.case.a(l)
            self._a[l] = (t.to(G.FP8) if self.sa is not None else t.to(self.dtype)).to(DEV)
        return self._a[l]

    @property
    def w8(self):
        if self._w8 is None:
            q, s = self.case.w8()
            self._w8 = (q.to(DEV), s.to(DEV), self.case.code_max())
        return self._w8


@functools.lru_cache(maxsize=6)
def _ops(M, N, Kd, dtype=BF16, fp8_act=False):
    return _Ops(M, N, Kd, dtype, fp8_act)


def _probe(o, epi, fn, what, pad=False, code_max=2.0, bias=None):
    """Run fn(a, bias, resid, out) once per layout of the case and check it against the exact result.
    bias: pass the bias (default: only under EPI_BIAS)."""
    c = o.case
    with_bias = (epi == EPI_BIAS) if bias is None else bias
    nout = c.N // 2 if epi == EPI_SWIGLU else c.N
    for l in range(c.L):
        a = G.padded(o.a(l)) if pad else o.a(l)
        resid = None
        if epi == EPI_RESID:
            resid = G.padded(o.resid) if pad else o.resid
        out = G.padded(torch.zeros(c.M, nout, dtype=o.dtype, device=DEV), extra=8) if pad else None
        got = fn(a, o.bias if with_bias else None, resid, out)
        ref = c.exact(l, epi, bias=with_bias)
        tag = f"{what} M={c.M} N={c.N} K={c.K} epi={epi} layout={l} pad={pad}"
        G.check_reference(ref, c.acc_max(l, code_max), o.dtype, epi, tag)
        G.check(got, ref, epi, tag)
    c.assert_covered()


def _epis(N, epis):
    return [e for e in epis if e != EPI_SWIGLU or N % 32 == 0]


def _plan(M, N, Kd, epi, **kw):
    return P.plan(M, N, Kd, epi, cus=K._cus(), **kw)


# ---------------------------------------------------------------------------------- M = 1
# N: gemm() takes N % 8 == 0 only (gemm_plan._plan), so the GEMV's narrow and ragged widths are 8 and
# 104 (26 four-row waves, a ragged last workgroup); gemm_w8 takes N % 4 == 0 and runs N = 4.
@pytest.mark.parametrize("Kd", [512, 1024, 4608, 8192])
@pytest.mark.parametrize("N", [8, 104, 544])
def test_gemv(N, Kd):
    """Tile 6, incl. the two-waves-per-row long-row form (narrow N at K >= 8192) and 2 / 3 layouts."""
    o = _ops(1, N, Kd)
    for epi in _epis(N, DECODE_EPIS):
        p = _plan(1, N, Kd, epi)
        assert (p.family, p.tile, p.splits) == ("gemv", P.TILE_GEMV, 1)
        for pad in (False, True):
            _probe(o, epi, lambda a, b, r, out: K.gemm(a, o.w, bias=b, epi=epi, resid=r, out=out), "gemv", pad)


@pytest.mark.parametrize("Kd", [1024, 3072, 8192])
@pytest.mark.parametrize("N", [4, 544])
def test_gemv_w8(N, Kd):
    o = _ops(1, N, Kd)
    wq, sw, cm = o.w8
    for epi in _epis(N, DECODE_EPIS):
        assert P.gemv_w8_fusable(1, N, Kd, epi) and P.weight_op("gemm", 1, N, Kd, epi) == "gemm_w8"
        _probe(o, epi, lambda a, b, r, out: K.gemm_w8(a, wq, sw, bias=b, epi=epi, resid=r, out=out), "gemm_w8",
               code_max=cm)


# ---------------------------------------------------------------------------------- 2..64 rows
@pytest.mark.parametrize("Kd", [256, 768, 3072])
@pytest.mark.parametrize("N", [16, 48, 3072])
def test_gemm_dk_and_w8(N, Kd):
    """gemm_dk (through gemm()'s hand-off and directly) and gemm_dk_w8: one and two 16-row blocks, the
    row after each block edge; BN 16 and the widest tile; one, three and twelve 256-wide K steps."""
    for M in (2, 15, 16, 17, 32):
        o = _ops(M, N, Kd)
        wq, sw, cm = o.w8
        for epi in _epis(N, DECODE_EPIS):
            assert _plan(M, N, Kd, epi) == P.plan_dk(M, N, Kd) == P.GemmPlan("dk", P.TILE_DK, 1, 0)
            assert P.plan_dk_w8(M, N, Kd).family == "dk_w8" and P.dk_w8_fusable(M, N, Kd, epi)
            assert P.weight_op("dk", M, N, Kd, epi) == "gemm_dk_w8"
            pad = M == 17
            _probe(o, epi, lambda a, b, r, out: K.gemm(a, o.w, bias=b, epi=epi, resid=r, out=out), "gemm->dk", pad)
            _probe(o, epi, lambda a, b, r, out: K.gemm_dk(a, o.w, epi=epi, bias=b, resid=r, out=out), "gemm_dk")
            _probe(o, epi, lambda a, b, r, out: K.gemm_dk_w8(a, wq, sw, epi=epi, bias=b, resid=r, out=out),
                   "gemm_dk_w8", pad, code_max=cm)


@pytest.mark.parametrize("Kd", [1024, 1536, 3072])
@pytest.mark.parametrize("N", [512, 1040])
def test_gemm_dk_splitk_and_w8(N, Kd):
    """33..64 rows: 64x128 partials at dk_splits + the reduce, bf16 and fp8 weights. K = 1536 is 24
    k-tiles: a split count with a factor 3."""
    for M in (33, 64):
        o = _ops(M, N, Kd)
        wq, sw, cm = o.w8
        p = P.plan_dk(M, N, Kd)
        assert (p.family, p.tile, p.splits) == ("dk_splitk", P.TILE_DK, P.dk_splits(N, Kd)) and p.splits >= 2
        assert (Kd != 1536 or p.splits % 3 == 0) and (Kd // 64) % p.splits == 0
        assert P.plan_dk_splitk_w8(M, N, Kd) == p
        for epi in (EPI_NONE, EPI_RESID):
            assert _plan(M, N, Kd, epi) == p
            pad = M == 33
            _probe(o, epi, lambda a, b, r, out: K.gemm_dk(a, o.w, epi=epi, bias=b, resid=r, out=out), "dk_splitk", pad)
            _probe(o, epi, lambda a, b, r, out: K.gemm_dk_splitk_w8(a, wq, sw, epi=epi, bias=b, resid=r, out=out),
                   "gemm_dk_splitk_w8", pad, code_max=cm)


# ---------------------------------------------------------------------------------- decode tiles
TILE_ROWS = [(P.TILE_32x128, 17), (P.TILE_64x128, 40), (P.TILE_64x128, 64), (P.TILE_64x128, 65),
             (P.TILE_128x64_PF4, 77), (P.TILE_128x64_PF4, 128)]
TILE_KS = [(64, 1), (192, 1), (320, 1), (768, 2), (768, 3), (3072, 4)]


@pytest.mark.parametrize("Kd,splits", TILE_KS, ids=[f"K{k}s{s}" for k, s in TILE_KS])
@pytest.mark.parametrize("N", [8, 136, 160, 392])
def test_gemm_decode_tiles(N, Kd, splits):
    """Tiles 2, 3 and 9 through gemm(tile=, splits=): one k-tile, 3 and 5 (fewer than and no multiple
    of the 4 in flight), split-K 2 / 3 / 4 + reduce. N = 160 carries the SwiGLU epilogue (N % 32)."""
    for tile, M in TILE_ROWS:
        o = _ops(M, N, Kd)
        for epi in _epis(N, DECODE_EPIS):
            p = _plan(M, N, Kd, epi, tile=tile, splits=splits)
            assert (p.family, p.tile, p.splits) == ("tile", tile, splits)
            _probe(o, epi, lambda a, b, r, out: K.gemm(a, o.w, bias=b, epi=epi, resid=r, out=out, tile=tile,
                                                       splits=splits), f"tile{tile}s{splits}", pad=M in (17, 65, 77))


@pytest.mark.parametrize("Kd", [192, 320, 768, 3072])
@pytest.mark.parametrize("N", [8, 136, 160, 392])
def test_gemm_tile_w8(N, Kd):
    """gemm_tile_w8 (K >= 128) on the tile and split count plan_tile_w8 gives it: tile 2 at 33..64 rows,
    tile 9 at 65..128."""
    for M, tile in ((40, P.TILE_64x128), (64, P.TILE_64x128), (65, P.TILE_128x64_PF4), (77, P.TILE_128x64_PF4),
                    (128, P.TILE_128x64_PF4)):
        o = _ops(M, N, Kd)
        wq, sw, cm = o.w8
        for epi in _epis(N, DECODE_EPIS):
            p = P.plan_tile_w8(M, N, Kd, epi, cus=K._cus())
            # a product gemm() hands to gemm_dk's split-K route keeps that route's split count
            want = P.dk_splits(N, Kd) if P.dk_fusable(M, N, Kd, epi) else P.auto_splits(M, N, Kd)
            assert (p.family, p.tile, p.splits) == ("tile", tile, want)
            _probe(o, epi, lambda a, b, r, out: K.gemm_tile_w8(a, wq, sw, epi=epi, bias=b, resid=r, out=out),
                   f"gemm_tile_w8 tile{tile}s{p.splits}", pad=M in (40, 77), code_max=cm)


@pytest.mark.parametrize("Kd", [320, 1024])
@pytest.mark.parametrize("M", [130, 261])
def test_gemm_auto_route_mid_rows(M, Kd):
    """129..639 rows, routed by the planner: the 64x128 tile over 3 / 5 row blocks, a ragged last one."""
    N = 264
    o = _ops(M, N, Kd)
    for epi in (EPI_NONE, EPI_RESID):
        p = _plan(M, N, Kd, epi)
        assert (p.family, p.tile, p.splits) == ("tile", P.TILE_64x128, P.auto_splits(M, N, Kd))
        for pad in (False, True):
            _probe(o, epi, lambda a, b, r, out: K.gemm(a, o.w, bias=b, epi=epi, resid=r, out=out), "auto", pad)


def _close(a, b, atol, rtol=0.02):
    a, b = a.float(), b.float()
    err = (a - b).abs()
    bad = (err > atol + rtol * b.abs()).sum().item()
    assert bad == 0, f"{bad} / {a.numel()} mismatches, max err {err.max().item():.4g}"


@pytest.mark.parametrize("Kd", [512, 3072])
@pytest.mark.parametrize("N", [512, 1032])
def test_gemm_resid_norm_and_w8(N, Kd):
    """out (the new residual rows) exact; h_out = RMSNorm(out) * gamma at the suite's tolerance."""
    g = (torch.randn(N, generator=torch.Generator().manual_seed(N + Kd)) + 1.0).to(BF16).to(DEV)
    for M, tile in ((2, P.TILE_32x128), (40, P.TILE_64x128), (64, P.TILE_64x128), (100, P.TILE_128x64_PF4)):
        o = _ops(M, N, Kd)
        p = P.plan_resid_norm(M, N, Kd)
        assert (p.family, p.tile, p.splits) == ("tile", tile, P.auto_splits(M, N, Kd))
        calls = [("gemm_resid_norm", 2.0, lambda a, x, h: K.gemm_resid_norm(a, o.w, x, g, 1e-5, out=x, h_out=h))]
        if M > P.TILE_W8_ABOVE:
            wq, sw, cm = o.w8
            assert P.plan_resid_norm_w8(M, N, Kd) == p
            calls.append(("gemm_resid_norm_w8", cm,
                          lambda a, x, h: K.gemm_resid_norm_w8(a, wq, sw, x, g, 1e-5, out=x, h_out=h)))
        for what, cm, call in calls:
            for pad in (False, M in (40, 100)):
                h_got = {}

                def fn(a, b, r, out):
                    x = G.padded(o.resid) if pad else o.resid.clone()
                    h_got["h"] = call(a, x, out)
                    return x
                _probe(o, EPI_RESID, fn, what, pad, code_max=cm)
                x_ref = o.resid.clone()
                h_ref = R.gemm_resid_norm(o.a(0), o.w, x_ref, g, 1e-5, out=x_ref)
                _close(h_got["h"], h_ref, atol=0.05)


# ---------------------------------------------------------------------------------- prefill tiles
def test_gemm_tile1_short_k():
    """640 rows at K = 64: the planner's 128x128 tile (one k-tile; gemm8p needs K >= 128)."""
    M, N, Kd = 640, 264, 64
    o = _ops(M, N, Kd)
    for epi in (EPI_NONE, EPI_BIAS):
        p = _plan(M, N, Kd, epi)
        assert (p.family, p.tile, p.splits) == ("tile", P.TILE_128x128, 1)
        for pad in (False, True):
            _probe(o, epi, lambda a, b, r, out: K.gemm(a, o.w, bias=b, epi=epi, resid=r, out=out), "tile1", pad)


PREFILL_MS = [129, 256, 257, 300]
PREFILL_NS = [8, 264, 288, 520]  # 288: the SwiGLU width (N % 32)
PREFILL_KS = [128, 192, 256, 320, 640]


@pytest.mark.parametrize("Kd", PREFILL_KS)
@pytest.mark.parametrize("tile", [P.TILE_8P_256, P.TILE_8P_128])
def test_gemm8p_tiles(tile, Kd):
    """Phase-split kernel, 256- and 128-row tiles: 2..10 k-tiles, one and two row / column tiles, ragged."""
    for M in PREFILL_MS:
        for N in PREFILL_NS:
            o = _ops(M, N, Kd)
            for epi in _epis(N, ALL_EPIS):
                p = _plan(M, N, Kd, epi, tile=tile, splits=1)
                assert (p.family, p.tile, p.splits) == ("gemm8p", tile, 1)
                _probe(o, epi, lambda a, b, r, out: K.gemm(a, o.w, bias=b, epi=epi, resid=r, out=out, tile=tile,
                                                           splits=1), f"gemm8p tile{tile}", pad=M == 257,
                       bias=epi in (EPI_BIAS, EPI_GELU))


@pytest.mark.parametrize("Kd", PREFILL_KS)
def test_gemm4w_variants(Kd):
    """Four-wave 256x256 kernel, schedules 0 / 1 / 2 (K / 64 even and >= 4 takes the variant; else two sets)."""
    prev = K.gemm4w_variant(-1)
    try:
        for v in (0, 1, 2):
            K.gemm4w_variant(v)
            for M in PREFILL_MS:
                for N in PREFILL_NS:
                    o = _ops(M, N, Kd)
                    for epi in _epis(N, ALL_EPIS):
                        p = _plan(M, N, Kd, epi, tile=P.TILE_4W, splits=1)
                        assert (p.family, p.tile, p.splits) == ("gemm4w", P.TILE_4W, 1)
                        _probe(o, epi, lambda a, b, r, out: K.gemm(a, o.w, bias=b, epi=epi, resid=r, out=out,
                                                                   tile=P.TILE_4W, splits=1), f"gemm4w v{v}",
                               pad=M == 300, bias=epi in (EPI_BIAS, EPI_GELU))
    finally:
        K.gemm4w_variant(prev)


@pytest.mark.parametrize("Kd", [128, 256])
@pytest.mark.parametrize("tile", [P.TILE_8P_256, P.TILE_8P_128])
def test_gemm8p_persistent_loop(tile, Kd):
    """More tiles than CUs (17 x 17 / 33 x 17): the persistent loop and one workgroup per tile."""
    M, N = 4100, 4104
    o = _ops(M, N, Kd)
    assert -(-M // 256) * -(-N // 256) > K._cus()
    prev = K.gemm8p_persist(-1)
    try:
        for on in (1, 0):
            K.gemm8p_persist(on)
            for epi in (EPI_NONE, EPI_RESID):
                p = _plan(M, N, Kd, epi, tile=tile, splits=1)
                assert (p.family, p.tile) == ("gemm8p", tile)
                _probe(o, epi, lambda a, b, r, out: K.gemm(a, o.w, bias=b, epi=epi, resid=r, out=out, tile=tile,
                                                           splits=1), f"gemm8p persist={on}")
    finally:
        K.gemm8p_persist(prev)


@pytest.mark.parametrize("Kd", [128, 256])
@pytest.mark.parametrize("H,Hkv,D", [(4, 4, 64), (8, 2, 128), (4, 2, 96)])
@pytest.mark.parametrize("M", [256, 300])
def test_gemm_rope(M, H, Hkv, D, Kd):
    """QKV + RoPE + KV-cache write in the gemm8p epilogue on angles that are multiples of 90 degrees
    (every rotation a swap / negation): q, k, v and both caches exact."""
    N = (H + 2 * Hkv) * D
    o = _ops(M, N, Kd)
    c = o.case
    assert M >= 256 and Kd % 64 == 0 and Kd >= 128  # gemm_rope's own kernel, not gemm + rope_cache
    S, L = 5, 1024
    g = torch.Generator().manual_seed(M + D)
    slot = torch.randint(0, S, (M,), generator=g, dtype=torch.int32)
    pos = torch.randperm(L, generator=g)[:M].to(torch.int32)
    cs = rope_table_90(L, D)
    for pad in (False, True):
        kc = torch.zeros(S, Hkv, L, D, device=DEV, dtype=BF16)
        vc = torch.zeros_like(kc)
        a = G.padded(o.a(0)) if pad else o.a(0)
        out = G.padded(torch.zeros(M, N, dtype=BF16, device=DEV), extra=8) if pad else None
        got = K.gemm_rope(a, o.w, pos.to(DEV), cs.to(DEV), H, Hkv, D, slot.to(DEV), kc, vc, out=out)
        ref, kc_ref, vc_ref = G.rope_exact(c, 0, pos, slot, cs, H, Hkv, D, torch.zeros(S, Hkv, L, D),
                                           torch.zeros(S, Hkv, L, D))
        for t in (ref, kc_ref, vc_ref):
            G.check_reference(t, c.acc_max(0))
        G.check(got, ref, what=f"gemm_rope qkv pad={pad}")
        G.check(kc, kc_ref, what="gemm_rope k cache")
        G.check(vc, vc_ref, what="gemm_rope v cache")
    c.assert_covered()


# ---------------------------------------------------------------------------------- W8A8 and fp16
@pytest.mark.parametrize("Kd", [128, 384, 1024])
@pytest.mark.parametrize("M", [129, 256, 300])
def test_gemm_fp8(M, Kd):
    """gemm256 (e4m3 x e4m3): aq = A in e4m3, per-row power-of-two sa, the fp8 copy of W."""
    for N in PREFILL_NS:
        o = _ops(M, N, Kd, fp8_act=True)
        wq, sw, cm = o.w8
        for epi in _epis(N, (EPI_NONE, EPI_GELU, EPI_SWIGLU, EPI_RESID)):
            # the decoder's prefill route; GELU is the fp8 encoder's MLP, which calls gemm_fp8 itself
            assert P.prefill_w8_fusable(M, N, Kd, epi) or (epi == EPI_GELU and Kd % 128 == 0 and N % 8 == 0)
            for pad in (False, M == 300):
                _probe(o, epi, lambda a, b, r, out: K.gemm_fp8(a, o.sa, wq, sw, bias=b, epi=epi, resid=r, out=out),
                       "gemm_fp8", pad, code_max=cm)

        def in_place(a, b, r, out):
            x = o.resid.clone()
            return K.gemm_fp8(a, o.sa, wq, sw, epi=EPI_RESID, resid=x, out=x)
        _probe(o, EPI_RESID, in_place, "gemm_fp8 in place", code_max=cm)


@pytest.mark.parametrize("Kd", [128, 320])
@pytest.mark.parametrize("N", [8, 264])
@pytest.mark.parametrize("M", [129, 300])
def test_gemm_f16(M, N, Kd):
    """The fp16 encoder GEMM (gemm8p's fp16 instance): fp16 holds every integer to 2048, so every
    element of these cases is exact."""
    o = _ops(M, N, Kd, dtype=F16)
    assert P.prefill_bm(M, N, K._cus()) in (128, 256)
    for epi in (EPI_NONE, EPI_BIAS, EPI_GELU, EPI_RESID):
        for pad in (False, M == 300):
            _probe(o, epi, lambda a, b, r, out: K.gemm_f16(a, o.w, bias=b, epi=epi, resid=r, out=out), "gemm_f16",
                   pad, bias=epi in (EPI_BIAS, EPI_GELU))
