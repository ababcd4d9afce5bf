"""Batch-1 GEMV on MXFP4 weights (csrc/gemv_w4.hip): exact-integer probes that see one wrong code,
nibble, scale byte or k-block; random operands vs the fp32 reference on the same codes and vs the
bf16 GEMV on the dequantised weights; what it writes; its refusals; and the decoder with
weight_dtype="mxfp4" (tiny, every product K = 1024; Phi-3 width, the production shapes)."""
import copy
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_probes as G  # noqa: E402
from test_gemv_w8_gpu import _near_argmax_under_reference, _reference_decoder  # noqa: E402

from docagents_amd.engine.generator import Generator  # noqa: E402
from docagents_amd.models.configs import decoder_config  # noqa: E402
from docagents_amd.models.llama import LlamaDecoder  # noqa: E402
from docagents_amd.ops import kernels as K  # noqa: E402
from docagents_amd.ops import reference as R  # noqa: E402

DEV = "cuda"
EPIS = [K.EPI_NONE, K.EPI_BIAS, K.EPI_RESID, K.EPI_SWIGLU]
LIVE = 1024  # live columns of A per launch: the reference alone then leaves <= 0.15 % of the outputs unrepresentable


def _rand(*shape, scale=1.0, dtype=torch.bfloat16):
    return (torch.randn(*shape, device=DEV) * scale).to(dtype)


def _close(a, b, atol, rtol=0.02):
    a, b = a.float(), b.float()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = (err > tol).sum().item()
    if a.numel():  # (8, 8192) SwiGLU rounds down to an empty product
        print(f"max err {err.max().item():.4g}, max err / tol {(err / tol).max().item():.3g}")
    assert bad == 0, f"{bad} / {a.numel()} mismatches, max err {err.max().item():.4g}"
    assert a.shape == b.shape


# ----------------------------------------------------------------------------------- exact probes
class W4Case:
    """Exact-integer operands in the style of gemm_probes.GemmCase, on the CPU: A is +-1 on the live
    columns of a layout, the codes are +-1 / +-2 (never 0), every MX block's scale byte is 127 or 128, so
    W is one of +-1, +-2, +-4 and one wrong code, nibble, scale byte or k-block moves an output by >= 1.
    K / 1024 layouts: the 64-column block j of A is live in layout j % (K / 1024)."""

    def __init__(self, N, Kd, seed=0):
        self.N, self.K, self.L = N, Kd, Kd // LIVE
        g = torch.Generator().manual_seed(seed * 1000003 + N * 104729 + Kd)
        self._a = (torch.randint(0, 2, (1, Kd), generator=g) * 2 - 1).double()
        mag = torch.randint(0, 2, (N, Kd), generator=g) * 2 + 2            # grid index 2 (1.0) or 4 (2.0)
        code = (mag | (torch.randint(0, 2, (N, Kd), generator=g) << 3)).to(torch.uint8)
        self.codes = (code[:, 0::2] | (code[:, 1::2] << 4)).contiguous()
        self.scales = torch.randint(127, 129, (N, Kd // 32), generator=g).to(torch.uint8)
        self.bias = torch.randint(-8, 9, (N,), generator=g).float()
        self.resid = torch.randint(-8, 9, (1, N), generator=g).float()
        self.w = R.dequant_mxfp4(self.codes, self.scales).double()
        assert set(self.w.abs().unique().tolist()) == {1.0, 2.0, 4.0}

    def live(self, l):
        return (torch.arange(self.K) // G.BLOCK) % self.L == l

    def a(self, l):
        return (self._a * self.live(l).double()[None]).float()

    def exact(self, l, epi, w=None):
        y = (self._a * self.live(l).double()[None]) @ (self.w if w is None else w).t()
        if epi == K.EPI_BIAS:
            y = y + self.bias.double()
        if epi == K.EPI_RESID:
            y = y + self.resid.double()
        return y


PROBE_SHAPES = [(96, 1024), (544, 3072), (1000, 5120), (3072, 8192), (8200, 1024)]


@pytest.mark.parametrize("N,Kd", PROBE_SHAPES)
def test_gemv_w4_exact_probes(N, Kd):
    c = W4Case(N, Kd)
    cover = torch.zeros(Kd, dtype=torch.int32)
    for l in range(c.L):
        assert int(c.live(l).sum()) == LIVE
        cover += c.live(l).int()
    assert bool((cover == 1).all()), "a column is live in no layout, or in two"
    q, s = c.codes.to(DEV), c.scales.to(DEV)
    bias, resid = c.bias.to(DEV, torch.bfloat16), c.resid.to(DEV, torch.bfloat16)
    worst = 0.0
    for l in range(c.L):
        a = c.a(l).to(DEV, torch.bfloat16)
        for epi in G.LINEAR:
            what = f"N={N} K={Kd} layout {l} epi {epi}"
            ref = c.exact(l, epi)
            G.check_reference(ref, LIVE * 4.0 + 8, epi=epi, what=what)
            worst = max(worst, G.rounded_mask(ref).double().mean().item())
            got = K.gemm_w4(a, q, s, bias=bias if epi == K.EPI_BIAS else None, epi=epi,
                            resid=resid if epi == K.EPI_RESID else None)
            G.check(got.cpu(), ref, epi, what)
    print(f"largest share of unrepresentable outputs in a launch: {worst:.4%}")


def test_exact_probes_see_two_swapped_scale_bytes():
    """Negative control, on the host: the exact result of a matrix whose row 5 has two scale bytes
    swapped (127 <-> 128) fails check() against the true one."""
    c = W4Case(96, 1024)
    row = c.scales[5]
    i, j = int((row == 127).nonzero()[0]), int((row == 128).nonzero()[0])
    bad = c.scales.clone()
    bad[5, i], bad[5, j] = c.scales[5, j], c.scales[5, i]
    wrong = c.exact(0, K.EPI_NONE, w=R.dequant_mxfp4(c.codes, bad).double())
    right = c.exact(0, K.EPI_NONE)
    G.check(right.to(torch.bfloat16), right)
    with pytest.raises(AssertionError):
        G.check(wrong.to(torch.bfloat16), right)


# ----------------------------------------------------------------------------------- random operands
def _operands(N, Kd, epi):
    if epi == K.EPI_SWIGLU:
        N = (N // 32) * 32
    w = _rand(N, Kd, scale=Kd ** -0.5)
    q, s = K.quant_weight_mxfp4(w)
    bias = _rand(N) if epi in (K.EPI_BIAS, K.EPI_RESID) else None
    resid = _rand(1, N) if epi == K.EPI_RESID else None
    return N, q, s, bias, resid


# one k-block; 3 blocks and N no multiple of the rows per workgroup; 5 blocks (no multiple of U or of a
# two-block load); two waves per row (with the tiny-N tail where waves own no row); the
# two-rows-per-wave dispatch arm; the LM head's row count
SHAPES = [(96, 1024), (544, 3072), (1000, 5120), (8, 8192), (3072, 8192), (8200, 1024), (32064, 1024)]


@pytest.mark.parametrize("N,Kd", SHAPES)
@pytest.mark.parametrize("epi", EPIS)
def test_gemv_w4_vs_fp32_reference(N, Kd, epi):
    """The reference holds the same quantised values: only the summation order and the final bf16
    rounding differ, so the bf16 GEMV tests' tolerance applies (atol 0.03, rtol 0.02, no mismatch)."""
    torch.manual_seed(N + Kd + epi)
    N, q, s, bias, resid = _operands(N, Kd, epi)
    kw = dict(bias=bias, epi=epi, resid=resid)
    a = _rand(1, Kd)
    got = K.gemm_w4(a, q, s, **kw)
    assert got.shape == (1, N // 2 if epi == K.EPI_SWIGLU else N) and got.dtype == torch.bfloat16
    _close(got, R.gemm_w4(a, q, s, **kw), atol=0.03)
    # fused RMSNorm, with a gain vector and with unit gain
    x, g = _rand(1, Kd, scale=3.0), _rand(Kd) + 1.0
    _close(K.gemm_w4(x, q, s, rms=(g, 1e-5), **kw), R.gemm_w4(x, q, s, rms=(g, 1e-5), **kw), atol=0.03)
    _close(K.gemm_w4(x, q, s, rms=(None, 1e-5), **kw), R.gemm_w4(x, q, s, rms=(None, 1e-5), **kw), atol=0.03)


@pytest.mark.parametrize("epi", EPIS)
def test_gemv_w4_scale_bytes_over_many_binades(epi):
    torch.manual_seed(17 + epi)
    N, q, _, bias, resid = _operands(544, 3072, epi)
    s = torch.randint(100, 141, (N, 3072 // 32), device=DEV).to(torch.uint8)
    a = _rand(1, 3072)
    kw = dict(bias=bias, epi=epi, resid=resid)
    _close(K.gemm_w4(a, q, s, **kw), R.gemm_w4(a, q, s, **kw), atol=0.03)


@pytest.mark.parametrize("N,Kd,epi", [(3072, 3072, K.EPI_NONE), (1024, 3072, K.EPI_SWIGLU), (3072, 8192, K.EPI_RESID)])
def test_gemv_w4_equals_bf16_gemv_on_dequantised_weights(N, Kd, epi):
    """Two schedules of one product: the dequantised weights are exact in bf16."""
    torch.manual_seed(N + Kd)
    N, q, s, _, resid = _operands(N, Kd, epi)
    dq = K.dequant_mxfp4(q, s)
    a = _rand(1, Kd)
    got = K.gemm_w4(a, q, s, epi=epi, resid=resid)
    _close(got, K.gemm(a, dq, epi=epi, resid=resid, tile=6, splits=1), atol=0.01)
    x = _rand(1, Kd, scale=3.0)
    _close(K.gemm_w4(x, q, s, epi=epi, resid=resid, rms=(None, 1e-5)),
           K.gemm(x, dq, epi=epi, resid=resid, tile=6, splits=1, rms=(None, 1e-5)), atol=0.01)


# ----------------------------------------------------------------------------------- writes
@pytest.mark.parametrize("N,Kd,epi", [(544, 3072, K.EPI_NONE), (1000, 5120, K.EPI_BIAS), (1024, 3072, K.EPI_SWIGLU),
                                      (3072, 8192, K.EPI_RESID)])
def test_gemv_w4_writes_only_its_outputs(N, Kd, epi):
    torch.manual_seed(N + epi)
    N, q, s, bias, resid = _operands(N, Kd, epi)
    a = _rand(1, Kd)
    nout = N // 2 if epi == K.EPI_SWIGLU else N
    pad = 64
    buf = torch.full((1, nout + 2 * pad), G.POISON, dtype=torch.bfloat16, device=DEV)
    out = buf[:, pad:pad + nout]
    operands = [t.clone() for t in (a, q, s)]
    got = K.gemm_w4(a, q, s, bias=bias, epi=epi, resid=resid, out=out)
    assert got.data_ptr() == out.data_ptr()
    _close(out, R.gemm_w4(a, q, s, bias=bias, epi=epi, resid=resid), atol=0.03)
    assert bool((buf[:, :pad] == G.POISON).all()) and bool((buf[:, pad + nout:] == G.POISON).all())
    assert all(torch.equal(t, u) for t, u in zip(operands, (a, q, s)))


def test_gemv_w4_in_place_residual():
    torch.manual_seed(5)
    N, q, s, _, resid = _operands(3072, 1024, K.EPI_RESID)
    a = _rand(1, 1024)
    want = R.gemm_w4(a, q, s, epi=K.EPI_RESID, resid=resid)
    x = resid.clone()
    out = K.gemm_w4(a, q, s, epi=K.EPI_RESID, resid=x, out=x)  # the decoder's x += a W^T
    assert out.data_ptr() == x.data_ptr()
    _close(x, want, atol=0.03)


# ----------------------------------------------------------------------------------- refusals
def test_gemm_w4_refusals(monkeypatch):
    """Anything the kernel would refuse raises ValueError on the host; nothing is launched."""
    def no_launch(*a, **kw):
        raise AssertionError("da_gemv_w4 launched")
    a = _rand(1, 1024)
    q, s = K.quant_weight_mxfp4(_rand(64, 1024))
    K.gemm_w4(a, q, s)  # accepted
    monkeypatch.setattr(K, "lib", lambda: type("L", (), {"da_gemv_w4": staticmethod(no_launch)})())
    q15, s15 = K.quant_weight_mxfp4(_rand(64, 1536))
    with pytest.raises(ValueError):
        K.gemm_w4(_rand(1, 1536), q15, s15)               # K % 1024
    with pytest.raises(ValueError):
        K.gemm_w4(_rand(2, 1024), q, s)                   # M = 2
    with pytest.raises(ValueError):
        K.gemm_w4(a, _rand(64, 512), s)                   # bf16 codes
    with pytest.raises(ValueError):
        K.gemm_w4(a, q.view(torch.float8_e4m3fn), s)      # fp8 codes
    q2, _ = K.quant_weight_mxfp4(_rand(64, 2048))
    with pytest.raises(ValueError):
        K.gemm_w4(a, q2[:, :512], s)                      # non-contiguous codes
    with pytest.raises(ValueError):
        K.gemm_w4(a, q, s[:, :16].contiguous())           # scale shape
    with pytest.raises(ValueError):
        K.gemm_w4(a, q, s[:32].contiguous())              # scale rows
    with pytest.raises(ValueError):
        K.gemm_w4(a, q, s.float())                        # scale dtype
    with pytest.raises(ValueError):
        K.gemm_w4(a, q[:48].contiguous(), s[:48].contiguous(), epi=K.EPI_SWIGLU)  # SwiGLU with N % 32
    with pytest.raises(ValueError):
        K.gemm_w4(a, q.cpu(), s)                          # host codes
    with pytest.raises(AssertionError, match="launched"):
        K.gemm_w4(a, q, s)                                # the patch is what an accepted call reaches


# ----------------------------------------------------------------------------------- model
class _Counting:
    def __init__(self, ops):
        self._ops, self.calls = ops, 0

    def __getattr__(self, name):
        return getattr(self._ops, name)

    def gemm_w4(self, *a, **kw):
        self.calls += 1
        return self._ops.gemm_w4(*a, **kw)


@pytest.fixture(scope="module")
def tiny_w4():
    cfg = decoder_config("tiny-dec-tp8")  # hidden 1024, FFN 1024: every product has K = 1024
    m = LlamaDecoder(cfg, "cuda", seed=11, weight_dtype="mxfp4")
    m.alloc_cache(3, 256)
    return m


def test_mxfp4_decoder_weights_are_the_dequantised_values(tiny_w4):
    m = tiny_w4
    n = 0
    for d, keys in [(L, ("wqkv", "wo", "w_gu", "w_down")) for L in m.w["layers"]] + [(m.w, ("lm_head",))]:
        for k in keys:
            q, e = d[k + "_q4"], d[k + "_e4"]
            assert q.dtype == torch.uint8 and e.dtype == torch.uint8 and d[k].dtype == torch.bfloat16
            assert q.is_cuda and torch.equal(d[k], R.dequant_mxfp4(q, e))
            n += 1
    assert n == 4 * m.cfg.layers + 1


def test_mxfp4_decoder_batch1_generation(tiny_w4):
    m = tiny_w4
    prompt = list(range(50, 83))
    a = Generator(m, max_batch=2, max_seq=256, temperature=0.0, use_graphs=True).generate([prompt], 10)[0]
    assert len(a.tokens) == 10
    _near_argmax_under_reference(_reference_decoder(m, 256), prompt, a.tokens)
    # the same model on the bf16 GEMVs (a deep copy of the weights; bf16 ignores the MXFP4 copies)
    u = LlamaDecoder(m.cfg, "cuda", weights=copy.deepcopy(m.w))
    u.alloc_cache(3, 256)
    u.ops = _Counting(u.ops)
    b = Generator(u, max_batch=2, max_seq=256, temperature=0.0, use_graphs=True).generate([prompt], 10)[0]
    assert u.ops.calls == 0
    print(a.tokens, b.tokens, a.mean_prob, b.mean_prob)
    assert sum(x == y for x, y in zip(a.tokens, b.tokens)) >= 8, (a.tokens, b.tokens)
    assert abs(a.mean_prob - b.mean_prob) < 0.05 * max(a.mean_prob, 1e-6) + 1e-4


def test_mxfp4_decoder_eager_step_runs_every_product_on_gemm_w4(tiny_w4, monkeypatch):
    m = tiny_w4
    monkeypatch.setattr(m, "ops", _Counting(m.ops))
    per_step = []
    step = m.decode_step

    def counted(st):
        c0 = m.ops.calls
        out = step(st)
        per_step.append(m.ops.calls - c0)
        return out
    monkeypatch.setattr(m, "decode_step", counted)
    g = Generator(m, max_batch=1, max_seq=256, temperature=0.0, use_graphs=False, share_prefix=False)
    g.generate([list(range(50, 83))], 3)
    assert per_step == [4 * m.cfg.layers + 1] * 2, per_step


def test_mxfp4_decoder_phi3_width():
    """Phi-3-mini at full width, 2 layers: the production GEMV shapes (9216 / 3072 / 16384 SwiGLU x
    3072, the two-wave 3072 x 8192 down projection, the 32064-row LM head)."""
    cfg = dataclasses.replace(decoder_config("phi3-mini"), layers=2)
    m = LlamaDecoder(cfg, "cuda", seed=5, weight_dtype="mxfp4")
    m.alloc_cache(3, 256)
    L = m.w["layers"][0]
    assert all(k + "_q4" in L and k + "_e4" in L for k in ("wqkv", "wo", "w_gu", "w_down")) and "lm_head_q4" in m.w
    prompt = [int(t) for t in np.random.default_rng(2).integers(5, 32000, size=64)]
    m.ops = _Counting(m.ops)
    out = Generator(m, max_batch=1, max_seq=256, temperature=0.0, use_graphs=True).generate([prompt], 8)[0]
    assert len(out.tokens) == 8 and m.ops.calls > 0
    _near_argmax_under_reference(_reference_decoder(m, 256), prompt, out.tokens)
