"""The decoder's MXFP4 weight form on the CPU: the quantiser (e2m1 codes, e8m0 block scales), the
reference route of the batch-1 products (reference.gemm_w4), the planner's answers, the decoder and
the startup checks of LLM_WEIGHT_DTYPE=mxfp4."""
import copy
import json
from pathlib import Path

import pytest
import torch

from docagents_amd import config
from docagents_amd.engine.generator import Generator
from docagents_amd.models.configs import decoder_config
from docagents_amd.models.llama import LlamaDecoder, TPContext
from docagents_amd.ops import gemm_plan as P
from docagents_amd.ops import kernels as K
from docagents_amd.ops import reference as R

MATS = ("wqkv", "wo", "w_gu", "w_down")
GRID = torch.tensor(R.E2M1_GRID)


def _matrix(N=64, Kd=1024, seed=7):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, Kd, generator=g) * Kd ** -0.5
    # blocks spread over many binades
    w = w * torch.exp2(torch.randint(-20, 21, (N, Kd // 32), generator=g).float()).repeat_interleave(32, dim=1)
    return w.to(torch.bfloat16)


def _nibbles(codes):
    """uint8 [N, K]: the code of every element, by the stated packing."""
    return torch.stack([codes & 0xF, codes >> 4], dim=-1).reshape(codes.shape[0], -1)


def _value(nib):
    v = GRID[(nib & 7).long()]
    return torch.where((nib & 8) != 0, -v, v)


def _expected_e(amax):
    """The smallest integer e with amax / 2^e <= 6 clamped to [-126, 127], 0 for amax = 0 (fp64 search)."""
    out = []
    for a in amax.double().flatten().tolist():
        if a == 0:
            out.append(0)
            continue
        e = -126
        while a / 2.0 ** e > 6 and e < 127:
            e += 1
        out.append(e)
    return torch.tensor(out).reshape(amax.shape)


def test_quantiser_shapes_codes_and_scale_bytes():
    w = _matrix()
    q, s = R.quant_weight_mxfp4(w)
    assert q.dtype == torch.uint8 and q.shape == (64, 512) and q.is_contiguous()
    assert s.dtype == torch.uint8 and s.shape == (64, 32) and s.is_contiguous()
    nib = _nibbles(q)
    assert not bool((nib == 0x8).any()), "negative zero stored"
    assert len(set(nib.flatten().tolist())) <= 15
    assert int(s.min()) >= 1 and int(s.max()) <= 254
    with pytest.raises(ValueError):
        R.quant_weight_mxfp4(torch.zeros(4, 48, dtype=torch.bfloat16))
    # kernels re-exports the same host-side functions
    assert K.quant_weight_mxfp4 is R.quant_weight_mxfp4 and K.dequant_mxfp4 is R.dequant_mxfp4


def test_quantiser_scale_rule_is_exact():
    w = _matrix().float()
    # amax exactly 6 * 2^e and 3 * 2^e; an all-zero block; amax 2^-130; a huge block; -0 elements
    w[0, :32] = 0.001; w[0, 5] = -6.0 * 2.0 ** -9
    w[1, 32:64] = 0.001; w[1, 40] = 3.0 * 2.0 ** 4
    w[2, :32] = 0
    w[3, :32] = 0; w[3, 7] = 2.0 ** -130
    w[4, :32] = 1.0; w[4, 1] = 2.0 ** 125
    w[5, :32] = -0.0
    w = w.to(torch.bfloat16)
    q, s = R.quant_weight_mxfp4(w)
    amax = w.float().reshape(64, 32, 32).abs().amax(-1)
    e = s.long() - 127
    assert torch.equal(e, _expected_e(amax))
    assert int(e[0, 0]) == -9 and int(e[1, 1]) == 3 and int(e[2, 0]) == 0 and int(e[3, 0]) == -126 and int(e[5, 0]) == 0
    nib = _nibbles(q)
    assert int(nib[0, 5]) == 0xF and int(nib[1, 40]) == 0x7           # -6 and +6 (3 * 2^4 = 6 * 2^3)
    assert not bool(nib[2, :32].any()) and not bool(nib[3, :32].any()) and not bool(nib[5, :32].any())
    assert int(s.min()) >= 1 and int(s.max()) <= 254 and not bool((nib == 0x8).any())
    assert bool(torch.isfinite(R.dequant_mxfp4(q, s).float()).all())


def test_quantiser_ties_round_to_the_even_mantissa_and_nibble_order():
    ties = {0.25: 0.0, 0.75: 1.0, 1.25: 1.0, 1.75: 2.0, 2.5: 2.0, 3.5: 4.0, 5.0: 4.0}
    w = torch.zeros(2, 32)
    w[:, 0] = 6.0  # e = 0 in both blocks
    for i, t in enumerate(ties):
        w[0, 1 + i], w[1, 1 + i] = t, -t
    w[0, 20], w[0, 21] = 1.0, -3.0  # byte 10: element 20 in bits 3:0, element 21 in bits 7:4
    q, s = R.quant_weight_mxfp4(w.to(torch.bfloat16))
    assert s.tolist() == [[127], [127]]
    val = _value(_nibbles(q))
    for i, (t, want) in enumerate(ties.items()):
        assert float(val[0, 1 + i]) == want and float(val[1, 1 + i]) == -want, (t, val[:, 1 + i])
    assert int(_nibbles(q)[1, 1]) == 0  # -0.25 rounds to zero: code 0, not -0
    assert int(q[0, 10]) == (0x2 | (0xD << 4))  # +1 = 0b0010, -3 = 0b1101
    assert int(q[0, 0]) == 0x7                  # element 0 = 6, element 1 = 0.25 -> 0


def test_dequantised_matrix_is_bf16_exact_and_within_format_error():
    w = _matrix()
    q, s = R.quant_weight_mxfp4(w)
    dq = R.dequant_mxfp4(q, s)
    assert dq.dtype == torch.bfloat16 and dq.shape == w.shape
    e = (s.long() - 127).repeat_interleave(32, dim=1)
    exact = _value(_nibbles(q)).double() * torch.exp2(e.double())
    assert torch.equal(dq.double(), exact)  # code value * 2^e, exactly, in bf16
    assert bool(((w.double() - dq.double()).abs() <= torch.exp2(e.double())).all())  # half the widest step (4 .. 6)


def test_requantising_the_dequantised_matrix():
    """The dequantised matrix is a fixed point: quantising it again dequantises to the same bits, and
    every block whose largest dequantised magnitude is still above 3 * 2^e keeps its codes and its
    scale byte. The stated scale rule (the SMALLEST e with amax / 2^e <= 6) cannot keep them elsewhere:
    a block with amax / 2^e in (3, 3.5) rounds to amax = 3 * 2^e, for which the rule gives e - 1 and
    the doubled codes (3 -> 6) — the same values — and a block that rounds to all zeros takes e = 0."""
    w = _matrix()
    q, s = R.quant_weight_mxfp4(w)
    dq = R.dequant_mxfp4(q, s)
    q2, s2 = R.quant_weight_mxfp4(dq)
    assert torch.equal(R.dequant_mxfp4(q2, s2), dq)
    e = s.double() - 127
    keeps = dq.double().reshape(64, 32, 32).abs().amax(-1) > 3 * torch.exp2(e)
    assert 0.5 < keeps.double().mean() < 1.0  # both kinds of block occur
    assert torch.equal(s2[keeps], s[keeps])
    assert torch.equal(q2.reshape(64, 32, 16)[keeps], q.reshape(64, 32, 16)[keeps])
    assert bool((s2[~keeps].long() == s[~keeps].long() - 1).all())
    # a third pass changes nothing at all
    q3, s3 = R.quant_weight_mxfp4(R.dequant_mxfp4(q2, s2))
    assert torch.equal(q3, q2) and torch.equal(s3, s2)


def test_reference_gemm_w4_is_the_product_on_the_dequantised_weights():
    g = torch.Generator().manual_seed(3)
    a = torch.randn(1, 1024, generator=g).to(torch.bfloat16)
    w = (torch.randn(64, 1024, generator=g) * 1024 ** -0.5).to(torch.bfloat16)
    q, s = R.quant_weight_mxfp4(w)
    dq = R.dequant_mxfp4(q, s)
    resid = torch.randn(1, 64, generator=g).to(torch.bfloat16)
    bias = torch.randn(64, generator=g).to(torch.bfloat16)
    gain = (torch.randn(1024, generator=g) + 1).to(torch.bfloat16)
    for epi, kw in ((R.EPI_NONE, {}), (R.EPI_BIAS, {"bias": bias}), (R.EPI_SWIGLU, {}),
                    (R.EPI_RESID, {"resid": resid}), (R.EPI_RESID, {"resid": resid, "bias": bias})):
        for rms in (None, (None, 1e-5), (gain, 1e-5)):
            got = R.gemm_w4(a, q, s, epi=epi, rms=rms, **kw)
            assert got.shape == (1, 32 if epi == R.EPI_SWIGLU else 64)
            assert torch.equal(got, R.gemm(a, dq, epi=epi, rms=rms, **kw))
    out = torch.empty(1, 64, dtype=torch.bfloat16)
    assert R.gemm_w4(a, q, s, out=out) is out and torch.equal(out, R.gemm(a, dq))


def test_planner_w4_truth_table():
    for mod in (P, R, K):  # the planner's objects, re-exported
        assert mod.gemv_w4_fusable is P.gemv_w4_fusable and mod.keeps_w4_copy is P.keeps_w4_copy
    for N, Kd, epi in ((9216, 3072, P.EPI_NONE), (3072, 3072, P.EPI_RESID), (16384, 3072, P.EPI_SWIGLU),
                       (3072, 8192, P.EPI_RESID), (32064, 3072, P.EPI_NONE), (64, 1024, P.EPI_BIAS),
                       (64, 1024, P.EPI_SWIGLU), (4, 1024, P.EPI_NONE)):
        assert P.gemv_w4_fusable(1, N, Kd, epi) and P.keeps_w4_copy(N, Kd, epi), (N, Kd, epi)
    assert not P.gemv_w4_fusable(1, 64, 1536) and not P.keeps_w4_copy(64, 1536)      # K % 1024
    assert not P.gemv_w4_fusable(2, 64, 1024) and P.keeps_w4_copy(64, 1024)          # M = 2: bf16, copy kept for M = 1
    assert not P.gemv_w4_fusable(0, 64, 1024)
    assert not P.gemv_w4_fusable(1, 48, 1024, P.EPI_SWIGLU) and not P.keeps_w4_copy(48, 1024, P.EPI_SWIGLU)
    assert not P.gemv_w4_fusable(1, 64, 1024, P.EPI_GELU) and not P.keeps_w4_copy(64, 1024, P.EPI_GELU)
    assert not P.gemv_w4_fusable(1, 62, 1024)                                          # N % 4


def test_weight_op_mxfp4_names_gemm_w4_only_at_one_row_on_the_gemm_body():
    shapes = ((9216, 3072, P.EPI_NONE), (3072, 3072, P.EPI_RESID), (16384, 3072, P.EPI_SWIGLU),
              (3072, 8192, P.EPI_RESID), (32064, 3072, P.EPI_NONE))
    bf16 = {"gemm": "gemm", "dk": "gemm_dk", "resid_norm": "gemm_resid_norm"}
    for N, Kd, epi in shapes:
        assert P.weight_op("gemm", 1, N, Kd, epi, weight_dtype="mxfp4") == "gemm_w4"
        for M in (2, 4, 16, 32, 33, 64, 96, 128, 129, 640, 2930):
            for body, name in bf16.items():
                assert P.weight_op(body, M, N, Kd, epi, weight_dtype="mxfp4") == name, (body, M, N, Kd)
        for body in ("dk", "resid_norm"):
            assert P.weight_op(body, 1, N, Kd, epi, weight_dtype="mxfp4") == bf16[body]
    assert P.weight_op("gemm", 1, 64, 1536, weight_dtype="mxfp4") == "gemm"
    assert P.weight_op("gemm", 1, 64, 1024, P.EPI_GELU, weight_dtype="mxfp4") == "gemm"
    with pytest.raises(ValueError):
        P.weight_op("nobody", 1, 64, 1024, weight_dtype="mxfp4")
    with pytest.raises(ValueError):
        P.weight_op("gemm", 1, 64, 1024, weight_dtype="int4")


def test_weight_op_without_the_keyword_keeps_the_golden_rows():
    routes = json.loads((Path(__file__).parent / "golden" / "w8_routes.json").read_text())["routes"]
    seen = set()
    for r in routes[::5]:
        for body in ("gemm", "dk", "resid_norm"):
            if body in r:
                assert P.weight_op(body, r["M"], r["N"], r["K"], r["epi"], ssq_out=r["ssq_out"]) == r[body], r
                assert P.weight_op(body, r["M"], r["N"], r["K"], r["epi"], ssq_out=r["ssq_out"],
                                   weight_dtype="fp8") == r[body], r
                seen.add(r[body])
    assert {"gemm_w8", "gemm_tile_w8", "gemm_dk_w8", "gemm_resid_norm_w8", "gemm"} <= seen, seen


class _Counting:
    """``ops`` with gemm_w4 counted (everything else passes through)."""

    def __init__(self, ops):
        self._ops, self.calls = ops, 0

    def __getattr__(self, name):
        return getattr(self._ops, name)

    def gemm_w4(self, *a, **kw):
        self.calls += 1
        return self._ops.gemm_w4(*a, **kw)


@pytest.fixture(scope="module")
def tiny_w4():
    cfg = decoder_config("tiny-dec-tp8")  # every product has K = 1024
    m = LlamaDecoder(cfg, "cpu", seed=3, weight_dtype="mxfp4")
    m.alloc_cache(3, 128)
    return cfg, m


def test_cpu_decoder_weights_are_the_dequantised_values_and_copies_are_kept(tiny_w4):
    cfg, m = tiny_w4
    n = 0
    for d in m.w["layers"] + [m.w]:
        for k in (MATS if d is not m.w else ("lm_head",)):
            q, e = d[k + "_q4"], d[k + "_e4"]
            N, Kd = d[k].shape
            assert q.dtype == torch.uint8 and q.shape == (N, Kd // 2) and e.dtype == torch.uint8 and e.shape == (N, Kd // 32)
            assert d[k].dtype == torch.bfloat16 and torch.equal(d[k], R.dequant_mxfp4(q, e))
            assert (k + "_q8") not in d
            n += 1
    assert n == 4 * cfg.layers + 1
    assert m.w["embed"].dtype == torch.bfloat16 and "embed_q4" not in m.w


def test_cpu_decoder_step_count_and_tokens_equal_bf16_on_dequantised_weights(tiny_w4, monkeypatch):
    cfg, m = tiny_w4
    b = LlamaDecoder(cfg, "cpu", weights=copy.deepcopy(m.w))  # weight_dtype="bf16" ignores the copies
    b.alloc_cache(3, 128)
    b.ops = _Counting(b.ops)
    monkeypatch.setattr(m, "ops", _Counting(m.ops))
    per_step = []
    step = m.decode_step

    def counted(st):
        c0 = m.ops.calls
        out = step(st)
        per_step.append(m.ops.calls - c0)
        return out
    monkeypatch.setattr(m, "decode_step", counted)
    prompt, new = list(range(40, 57)), 5
    got = Generator(m, max_batch=1, max_seq=128, temperature=0.0, use_graphs=False, share_prefix=False).generate([prompt], new)[0]
    want = Generator(b, max_batch=1, max_seq=128, temperature=0.0, use_graphs=False, share_prefix=False).generate([prompt], new)[0]
    assert per_step == [4 * cfg.layers + 1] * (new - 1), per_step
    assert b.ops.calls == 0
    assert len(got.tokens) == new and got.tokens == want.tokens


def test_mxfp4_startup_checks():
    cfg = decoder_config("tiny-dec-tp8")
    with pytest.raises(ValueError, match="weight_dtype"):
        LlamaDecoder(cfg, "cpu", weight_dtype="int4")
    with pytest.raises(ValueError, match="TP"):
        LlamaDecoder(cfg, "cpu", tp=TPContext(0, 2), weight_dtype="mxfp4")
    with pytest.raises(ValueError, match="prefill_dtype='fp8' needs weight_dtype='fp8'"):
        LlamaDecoder(cfg, "cpu", weight_dtype="mxfp4", prefill_dtype="fp8")
    assert LlamaDecoder(cfg, "cpu", weight_dtype="mxfp4", kv_dtype="fp8").kv_dtype == "fp8"
    assert config.load({"LLM_WEIGHT_DTYPE": "mxfp4"}).validate_engine().llm_weight_dtype == "mxfp4"
    c = config.load({"LLM_WEIGHT_DTYPE": "mxfp4", "KV_CACHE_DTYPE": "fp8"}).validate_engine()
    assert (c.llm_weight_dtype, c.kv_cache_dtype) == ("mxfp4", "fp8")
    with pytest.raises(ValueError, match="TP_SIZE"):
        config.load({"LLM_WEIGHT_DTYPE": "mxfp4", "TP_SIZE": "2"}).validate_engine()
    with pytest.raises(ValueError, match="LLM_PREFILL_DTYPE=fp8 needs LLM_WEIGHT_DTYPE=fp8"):
        config.load({"LLM_WEIGHT_DTYPE": "mxfp4", "LLM_PREFILL_DTYPE": "fp8"}).validate_engine()
    with pytest.raises(ValueError, match="LLM_WEIGHT_DTYPE"):
        config.load({"LLM_WEIGHT_DTYPE": "int4"}).validate_engine()


def test_engine_mxfp4_decoder_answers_on_cpu():
    from docagents_amd.engine.engine import Engine
    e = Engine("tiny-enc", "tiny-dec-tp8", "cpu", max_batch=2, max_seq=512, max_new_tokens=4, summary_max_new=4,
               temperature=0.0, use_graphs=False, load_encoder=False, llm_weight_dtype="mxfp4")
    assert e.decoder.weight_dtype == "mxfp4" and "wqkv_q4" in e.decoder.w["layers"][0]
    e.decoder.ops = _Counting(e.decoder.ops)
    text, conf = e.answer_text("what is this?", "some context words", 0.5)
    assert isinstance(text, str) and 0.0 <= conf <= 1.0
    assert e.decoder.ops.calls > 0
