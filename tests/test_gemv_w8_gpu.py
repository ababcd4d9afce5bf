"""Batch-1 GEMV on fp8 (e4m3) weights (csrc/gemv_w8.hip) vs the fp32 reference on the same quantised
values, vs the bf16 GEMV on the dequantised weights, its refusals, and the decoder with
weight_dtype="fp8" (tiny, every product K = 1024; Phi-3 width, the production shapes)."""
import copy
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from docagents_amd.engine.generator import Generator  # noqa: E402
from docagents_amd.models.configs import decoder_config  # noqa: E402
from docagents_amd.models.llama import LlamaDecoder  # noqa: E402
from docagents_amd.ops import kernels as K  # noqa: E402
from docagents_amd.ops import reference as R  # noqa: E402

DEV = "cuda"
EPIS = [K.EPI_NONE, K.EPI_BIAS, K.EPI_RESID, K.EPI_SWIGLU]


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


def _operands(N, Kd, epi):
    if epi == K.EPI_SWIGLU:
        N = (N // 32) * 32
    w = _rand(N, Kd, scale=Kd ** -0.5)
    q, s = K.quant_weight_fp8_pow2(w)
    bias = _rand(N) if epi in (K.EPI_BIAS, K.EPI_RESID) else None
    resid = _rand(1, N) if epi == K.EPI_RESID else None
    return N, q, s, bias, resid


# one k-block; 3 blocks and N no multiple of the rows per workgroup; blocks no multiple of U; two
# waves per row (with the tiny-N tail where waves own no row); the two-rows-per-wave dispatch arm
SHAPES = [(96, 1024), (544, 3072), (1000, 5120), (8, 8192), (3072, 8192), (8200, 1024), (32064, 1024)]


@pytest.mark.parametrize("N,Kd", SHAPES)
@pytest.mark.parametrize("epi", EPIS)
def test_gemv_w8_vs_fp32_reference(N, Kd, epi):
    """The reference holds the same quantised values: only the summation order and the final bf16
    rounding differ, so the bf16 GEMV tests' tolerance applies (atol 0.03, rtol 0.02, no mismatch)."""
    torch.manual_seed(N + Kd + epi)
    N, q, s, bias, resid = _operands(N, Kd, epi)
    kw = dict(bias=bias, epi=epi, resid=resid)
    a = _rand(1, Kd)
    got = K.gemm_w8(a, q, s, **kw)
    assert got.shape == (1, N // 2 if epi == K.EPI_SWIGLU else N) and got.dtype == torch.bfloat16
    _close(got, R.gemm_w8(a, q, s, **kw), atol=0.03)
    # arbitrary fp32 row scales
    s2 = (s * (0.5 + 1.5 * torch.rand(N, device=DEV))).contiguous()
    _close(K.gemm_w8(a, q, s2, **kw), R.gemm_w8(a, q, s2, **kw), atol=0.03)
    # fused RMSNorm, with a gain vector and with unit gain
    x, g = _rand(1, Kd, scale=3.0), _rand(Kd) + 1.0
    _close(K.gemm_w8(x, q, s, rms=(g, 1e-5), **kw), R.gemm_w8(x, q, s, rms=(g, 1e-5), **kw), atol=0.03)
    _close(K.gemm_w8(x, q, s, rms=(None, 1e-5), **kw), R.gemm_w8(x, q, s, rms=(None, 1e-5), **kw), atol=0.03)


def test_gemv_w8_writes_into_out_and_in_place_residual():
    torch.manual_seed(5)
    N, q, s, _, resid = _operands(3072, 1024, K.EPI_RESID)
    a = _rand(1, 1024)
    want = R.gemm_w8(a, q, s, epi=K.EPI_RESID, resid=resid)
    x = resid.clone()
    out = K.gemm_w8(a, q, s, epi=K.EPI_RESID, resid=x, out=x)  # the decoder's x += a W^T
    assert out.data_ptr() == x.data_ptr()
    _close(x, want, atol=0.03)


@pytest.mark.parametrize("N,Kd,epi", [(3072, 3072, K.EPI_NONE), (1024, 3072, K.EPI_SWIGLU), (3072, 8192, K.EPI_RESID)])
def test_gemv_w8_equals_bf16_gemv_on_dequantised_weights(N, Kd, epi):
    """Two schedules of one product: the dequantised weights are exact in bf16."""
    torch.manual_seed(N + Kd)
    N, q, s, _, resid = _operands(N, Kd, epi)
    dq = (q.float() * s[:, None]).to(torch.bfloat16)
    assert torch.equal(dq.float(), q.float() * s[:, None])
    a = _rand(1, Kd)
    got = K.gemm_w8(a, q, s, epi=epi, resid=resid)
    _close(got, K.gemm(a, dq, epi=epi, resid=resid, tile=6, splits=1), atol=0.01)
    x = _rand(1, Kd, scale=3.0)
    _close(K.gemm_w8(x, q, s, epi=epi, resid=resid, rms=(None, 1e-5)),
           K.gemm(x, dq, epi=epi, resid=resid, tile=6, splits=1, rms=(None, 1e-5)), atol=0.01)


def test_gemm_w8_refusals(monkeypatch):
    """Anything the kernel would refuse raises ValueError on the host; nothing is launched."""
    def no_launch(*a, **kw):
        raise AssertionError("da_gemv_w8 launched")
    lib = K.lib()
    a = _rand(1, 1024)
    q, s = K.quant_weight_fp8_pow2(_rand(64, 1024))
    K.gemm_w8(a, q, s)  # accepted
    monkeypatch.setattr(K, "lib", lambda: type("L", (), {"da_gemv_w8": staticmethod(no_launch)})())
    q15, s15 = K.quant_weight_fp8_pow2(_rand(64, 1536))
    with pytest.raises(ValueError):
        K.gemm_w8(_rand(1, 1536), q15, s15)               # K % 1024
    with pytest.raises(ValueError):
        K.gemm_w8(_rand(2, 1024), q, s)                   # M = 2
    with pytest.raises(ValueError):
        K.gemm_w8(a, _rand(64, 1024), s)                  # bf16 wq
    q2, _ = K.quant_weight_fp8_pow2(_rand(64, 2048))
    with pytest.raises(ValueError):
        K.gemm_w8(a, q2[:, :1024], s)                     # non-contiguous wq
    with pytest.raises(ValueError):
        K.gemm_w8(a, q, s[:32])                           # scale length
    with pytest.raises(ValueError):
        K.gemm_w8(a, q[:48], s[:48].contiguous(), epi=K.EPI_SWIGLU)  # SwiGLU with N % 32
    assert not K.gemv_w8_fusable(2, 64, 1024) and not K.gemv_w8_fusable(1, 64, 1536)
    assert not K.gemv_w8_fusable(1, 48, 1024, K.EPI_SWIGLU) and not K.gemv_w8_fusable(1, 64, 1024, K.EPI_GELU)
    assert K.gemv_w8_fusable(1, 64, 1024, K.EPI_SWIGLU)
    del lib


# ----------------------------------------------------------------------------------- model
def _near_argmax_under_reference(r, prompt, gen, margin=0.1):
    """Teacher-forced check of a generated sequence against the fp32 reference model: every token the
    HIP path chose is within ``margin`` (log-prob) of the reference's best token given the same
    history (a wrong kernel picks tokens several nats below the best)."""
    worst = 0.0
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    for t, tok in enumerate(gen):
        seq = prompt + gen[:t]
        flat = np.asarray(seq, dtype=np.int32)
        lg = r.prefill(to(flat), to(np.arange(len(seq), dtype=np.int32)), to(np.zeros(len(seq), dtype=np.int32)),
                       to(np.array([0, len(seq)], dtype=np.int32)), len(seq), to(np.array([len(seq) - 1])))
        lp = torch.log_softmax(lg[0].float(), -1)
        worst = max(worst, float(lp.max() - lp[tok]))
    print(f"worst log-prob gap to the reference's best token: {worst:.4g}")
    assert worst <= margin, worst
    return worst


class _Counting:
    def __init__(self, ops):
        self._ops, self.calls = ops, 0

    def __getattr__(self, name):
        return getattr(self._ops, name)

    def gemm_w8(self, *a, **kw):
        self.calls += 1
        return self._ops.gemm_w8(*a, **kw)


def _reference_decoder(m, max_seq):
    r = LlamaDecoder(m.cfg, "cuda", weights=m.w)  # weight_dtype="bf16": the (dequantised) bf16 tensors
    r.ops = R
    r.alloc_cache(2, max_seq)
    return r


@pytest.fixture(scope="module")
def tiny_fp8():
    cfg = decoder_config("tiny-dec-tp8")  # hidden 1024, FFN 1024: every product has K = 1024
    m = LlamaDecoder(cfg, "cuda", seed=11, weight_dtype="fp8")
    m.alloc_cache(3, 256)
    return m


def test_fp8_decoder_weights_are_the_dequantised_values(tiny_fp8):
    m = tiny_fp8
    n = 0
    for d, keys in [(L, ("wqkv", "wo", "w_gu", "w_down")) for L in m.w["layers"]] + [(m.w, ("lm_head",))]:
        for k in keys:
            q, s = d[k + "_q8"], d[k + "_s8"]
            assert q.dtype == torch.float8_e4m3fn and s.dtype == torch.float32 and d[k].dtype == torch.bfloat16
            assert torch.equal(d[k].float(), q.float() * s[:, None])
            n += 1
    assert n == 4 * m.cfg.layers + 1


def test_fp8_decoder_batch1_generation(tiny_fp8):
    m = tiny_fp8
    prompt = list(range(50, 83))
    a = Generator(m, max_batch=2, max_seq=256, temperature=0.0, use_graphs=True).generate([prompt], 10)[0]
    assert len(a.tokens) == 10
    _near_argmax_under_reference(_reference_decoder(m, 256), prompt, a.tokens)
    # the same model on the bf16 GEMVs (a deep copy of the weights; bf16 ignores the fp8 copies)
    u = LlamaDecoder(m.cfg, "cuda", weights=copy.deepcopy(m.w))
    u.alloc_cache(3, 256)
    u.ops = _Counting(u.ops)
    b = Generator(u, max_batch=2, max_seq=256, temperature=0.0, use_graphs=True).generate([prompt], 10)[0]
    assert u.ops.calls == 0
    print(a.tokens, b.tokens, a.mean_prob, b.mean_prob)
    assert sum(x == y for x, y in zip(a.tokens, b.tokens)) >= 8, (a.tokens, b.tokens)
    assert abs(a.mean_prob - b.mean_prob) < 0.05 * max(a.mean_prob, 1e-6) + 1e-4


def test_fp8_decoder_eager_step_runs_every_product_on_gemm_w8(tiny_fp8, monkeypatch):
    m = tiny_fp8
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


def test_fp8_decoder_phi3_width():
    """Phi-3-mini at full width, 2 layers: the production GEMV shapes (9216 / 3072 / 16384 SwiGLU x
    3072, the two-wave 3072 x 8192 down projection, the 32064-row LM head)."""
    cfg = dataclasses.replace(decoder_config("phi3-mini"), layers=2)
    m = LlamaDecoder(cfg, "cuda", seed=5, weight_dtype="fp8")
    m.alloc_cache(3, 256)
    L = m.w["layers"][0]
    assert all(k + "_q8" in L for k in ("wqkv", "wo", "w_gu", "w_down")) and "lm_head_q8" in m.w
    prompt = [int(t) for t in np.random.default_rng(2).integers(5, 32000, size=64)]
    m.ops = _Counting(m.ops)
    out = Generator(m, max_batch=1, max_seq=256, temperature=0.0, use_graphs=True).generate([prompt], 8)[0]
    assert len(out.tokens) == 8 and m.ops.calls > 0
    _near_argmax_under_reference(_reference_decoder(m, 256), prompt, out.tokens)
