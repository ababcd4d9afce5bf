"""The decoder's fp8 (e4m3) weight form on the CPU: the power-of-two row quantiser, the reference
route of the batch-1 products (reference.gemm_w8), and the startup checks of LLM_WEIGHT_DTYPE."""
import copy

import pytest
import torch

from docagents_amd import config
from docagents_amd.engine.generator import Generator
from docagents_amd.models.configs import decoder_config
from docagents_amd.models.llama import LlamaDecoder, TPContext
from docagents_amd.ops import reference as R

FP8 = torch.float8_e4m3fn
MATS = ("wqkv", "wo", "w_gu", "w_down")


def _matrix():
    g = torch.Generator().manual_seed(7)
    return (torch.randn(64, 1024, generator=g) * 1024 ** -0.5).to(torch.bfloat16)


def test_quantiser_scales_are_powers_of_two_in_range():
    w = _matrix()
    q, s = R.quant_weight_fp8_pow2(w)
    assert q.dtype == FP8 and q.shape == w.shape and s.dtype == torch.float32 and s.shape == (64,)
    mant, _ = torch.frexp(s)
    assert torch.all(mant == 0.5), s
    ratio = w.float().abs().amax(dim=1) / s
    assert torch.all(ratio > 224) and torch.all(ratio <= 448), ratio
    # rows spread over many binades, and amax exactly at a power of two times 448
    scale = torch.exp2(torch.arange(-30, 34, dtype=torch.float32))[:, None]
    w2 = (w.float() * scale).to(torch.bfloat16)
    w2[5, 0] = 448.0 * 2.0 ** -25
    w2[5, 1:] = 0
    q2, s2 = R.quant_weight_fp8_pow2(w2)
    assert torch.all(torch.frexp(s2)[0] == 0.5)
    r2 = w2.float().abs().amax(dim=1) / s2
    assert torch.all(r2 > 224) and torch.all(r2 <= 448), r2
    assert float(s2[5]) == 2.0 ** -25 and float(q2[5, 0].float()) == 448.0


def test_quantiser_dequantised_matrix_is_bf16_exact_and_within_format_error():
    w = _matrix()
    q, s = R.quant_weight_fp8_pow2(w)
    dq = q.float() * s[:, None]
    assert torch.equal(dq.to(torch.bfloat16).float(), dq)
    # e4m3: 3 mantissa bits (relative error <= 2^-4), subnormal step 2^-9 (absolute error <= 2^-10 s)
    err = (dq - w.float()).abs()
    bound = torch.maximum(2.0 ** -4 * w.float().abs(), 2.0 ** -10 * s[:, None].expand_as(dq))
    assert torch.all(err <= bound), float((err - bound).max())


def test_quantiser_zero_row():
    w = _matrix()
    w[3] = 0
    q, s = R.quant_weight_fp8_pow2(w)
    assert float(s[3]) == 1.0 and torch.all(q[3].float() == 0)
    assert torch.all(torch.isfinite(q.float()))


def test_kernel_and_reference_quantisers_agree():
    from docagents_amd.ops import kernels as K
    w = _matrix()
    (qa, sa), (qb, sb) = K.quant_weight_fp8_pow2(w), R.quant_weight_fp8_pow2(w)
    assert torch.equal(qa.float(), qb.float()) and torch.equal(sa, sb)


def test_reference_gemm_w8_is_the_product_on_the_dequantised_weights():
    g = torch.Generator().manual_seed(3)
    a = torch.randn(1, 1024, generator=g).to(torch.bfloat16)
    w = _matrix()
    q, s = R.quant_weight_fp8_pow2(w)
    dq = (q.float() * s[:, None]).to(torch.bfloat16)
    resid = torch.randn(1, 64, generator=g).to(torch.bfloat16)
    for epi, kw in ((R.EPI_NONE, {}), (R.EPI_SWIGLU, {}), (R.EPI_RESID, {"resid": resid})):
        for rms in (None, (None, 1e-5)):
            assert torch.equal(R.gemm_w8(a, q, s, epi=epi, rms=rms, **kw), R.gemm(a, dq, epi=epi, rms=rms, **kw))
    assert R.gemv_w8_fusable(1, 64, 1024) and not R.gemv_w8_fusable(2, 64, 1024)
    assert not R.gemv_w8_fusable(1, 64, 1536)


class _Counting:
    """``ops`` with gemm_w8 counted (everything else passes through)."""

    def __init__(self, ops):
        self._ops, self.calls = ops, 0

    def __getattr__(self, name):
        return getattr(self._ops, name)

    def gemm_w8(self, *a, **kw):
        self.calls += 1
        return self._ops.gemm_w8(*a, **kw)


def _tiny_fp8():
    cfg = decoder_config("tiny-dec-tp8")
    m = LlamaDecoder(cfg, "cpu", seed=3, weight_dtype="fp8")
    m.alloc_cache(3, 128)
    return cfg, m


def test_cpu_decoder_fp8_generates_through_gemm_w8_and_equals_bf16_on_dequantised_weights():
    cfg, m = _tiny_fp8()
    for d in m.w["layers"] + [m.w]:
        for k in (MATS if d is not m.w else ("lm_head",)):
            q, s = d[k + "_q8"], d[k + "_s8"]
            assert q.dtype == FP8 and q.shape == d[k].shape and s.shape == (d[k].shape[0],)
            assert d[k].dtype == torch.bfloat16 and torch.equal(d[k].float(), q.float() * s[:, None])
    assert m.w["embed"].dtype == torch.bfloat16 and "embed_q8" not in m.w
    # the bf16 decoder on the same (dequantised) weights: weight_dtype="bf16" ignores the fp8 copies
    b = LlamaDecoder(cfg, "cpu", weights=copy.deepcopy(m.w))
    b.alloc_cache(3, 128)
    b.ops = _Counting(b.ops)
    m.ops = _Counting(m.ops)
    prompt = list(range(40, 57))
    new = 5
    got = Generator(m, max_batch=1, max_seq=128, temperature=0.0, use_graphs=False).generate([prompt], new)[0]
    want = Generator(b, max_batch=1, max_seq=128, temperature=0.0, use_graphs=False).generate([prompt], new)[0]
    assert len(got.tokens) == new
    assert m.ops.calls >= (new - 1) * (4 * cfg.layers + 1), m.ops.calls  # every decode step's products
    assert b.ops.calls == 0
    assert got.tokens == want.tokens


def test_weight_dtype_startup_checks():
    cfg = decoder_config("tiny-dec-tp8")
    with pytest.raises(ValueError, match="weight_dtype"):
        LlamaDecoder(cfg, "cpu", weight_dtype="int4")
    with pytest.raises(ValueError, match="TP"):
        LlamaDecoder(cfg, "cpu", tp=TPContext(0, 2), weight_dtype="fp8")
    assert config.load({}).validate_engine().llm_weight_dtype == "bf16"
    assert config.load({"LLM_WEIGHT_DTYPE": "fp8"}).validate_engine().llm_weight_dtype == "fp8"
    with pytest.raises(ValueError, match="LLM_WEIGHT_DTYPE"):
        config.load({"LLM_WEIGHT_DTYPE": "int4"}).validate_engine()
    with pytest.raises(ValueError, match="TP_SIZE"):
        config.load({"LLM_WEIGHT_DTYPE": "fp8", "TP_SIZE": "2"}).validate_engine()


def test_engine_fp8_decoder_answers_on_cpu():
    from docagents_amd.engine.engine import Engine
    e = Engine("tiny-enc", "tiny-dec-tp8", "cpu", max_batch=2, max_seq=512, max_new_tokens=4, summary_max_new=4,
               temperature=0.0, use_graphs=False, load_encoder=False, llm_weight_dtype="fp8")
    assert e.decoder.weight_dtype == "fp8" and "wqkv_q8" in e.decoder.w["layers"][0]
    e.decoder.ops = _Counting(e.decoder.ops)
    text, conf = e.answer_text("what is this?", "some context words", 0.5)
    assert isinstance(text, str) and 0.0 <= conf <= 1.0
    assert e.decoder.ops.calls > 0
