"""The decoder with weight_dtype="fp8" at 2..32 rows: every gemm_dk product of a step streams the
e4m3 copy (ops.gemm_dk_w8); 33..64 rows and the bf16 decoder never do."""
import copy
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from docagents_amd.engine.generator import Generator  # noqa: E402
from docagents_amd.models.configs import decoder_config  # noqa: E402
from docagents_amd.models.llama import DecodeState, LlamaDecoder  # noqa: E402

from test_gemv_w8_gpu import _near_argmax_under_reference, _reference_decoder  # noqa: E402


class _Counting:
    def __init__(self, ops):
        self._ops, self.w8, self.dk = ops, 0, 0

    def __getattr__(self, name):
        return getattr(self._ops, name)

    def gemm_dk_w8(self, *a, **kw):
        self.w8 += 1
        return self._ops.gemm_dk_w8(*a, **kw)

    def gemm_dk(self, *a, **kw):
        self.dk += 1
        return self._ops.gemm_dk(*a, **kw)


@pytest.fixture(scope="module")
def tiny_fp8():
    m = LlamaDecoder(decoder_config("tiny-dec-tp8"), "cuda", seed=11, weight_dtype="fp8")  # hidden 1024
    m.alloc_cache(48, 128)
    return m


def test_fp8_decoder_batch4_generation(tiny_fp8):
    m = tiny_fp8
    prompts = [list(range(50, 83)), list(range(300, 317)), list(range(1000, 1041)), list(range(7, 30))]
    a = Generator(m, max_batch=4, max_seq=128, temperature=0.0, use_graphs=True).generate(prompts, 8)
    assert [len(r.tokens) for r in a] == [8] * 4
    ref = _reference_decoder(m, 128)
    for p, r in zip(prompts, a):
        _near_argmax_under_reference(ref, p, r.tokens)
    # the same model on the bf16 gemm_dk (a deep copy of the weights; bf16 ignores the fp8 copies)
    u = LlamaDecoder(m.cfg, "cuda", weights=copy.deepcopy(m.w))
    u.alloc_cache(5, 128)
    u.ops = _Counting(u.ops)
    b = Generator(u, max_batch=4, max_seq=128, temperature=0.0, use_graphs=True).generate(prompts, 8)
    assert u.ops.w8 == 0 and u.ops.dk > 0
    for x, y in zip(a, b):
        print(x.tokens, y.tokens)
        assert sum(s == t for s, t in zip(x.tokens, y.tokens)) >= 0.8 * 8, (x.tokens, y.tokens)


def _eager_step(m, B):
    """Calls of (gemm_dk_w8, gemm_dk) in one eager decode step over B rows (slots 0 .. B-1, position 1)."""
    st = DecodeState(m, B, 4, 0.0, 0)
    st.slot.copy_(torch.arange(B, dtype=torch.int32))
    st.pos.fill_(1)
    st.lens.fill_(2)
    st.active.fill_(1)
    st.tokens.copy_(torch.arange(5, 5 + B, dtype=torch.int32))
    ops = m.ops
    m.ops = c = _Counting(ops)
    try:
        m.decode_step(st)
        torch.cuda.synchronize()
    finally:
        m.ops = ops
    return c.w8, c.dk


def test_fp8_decoder_op_counts(tiny_fp8):
    m = tiny_fp8
    assert _eager_step(m, 4) == (4 * m.cfg.layers + 1, 0)
    assert _eager_step(m, 40)[0] == 0  # 33..64 rows stay on the bf16 tensors
    u = LlamaDecoder(m.cfg, "cuda", weights=copy.deepcopy(m.w))
    u.alloc_cache(5, 128)
    assert _eager_step(u, 4) == (0, 4 * m.cfg.layers + 1)


def test_fp8_decoder_phi3_width_batch16():
    """Phi-3-mini at full width, 2 layers, 16 rows: the production shapes (9216 / 3072 / 16384 SwiGLU
    x 3072, 3072 x 8192, the 32064-row LM head) with the deferred norms chained through them."""
    cfg = dataclasses.replace(decoder_config("phi3-mini"), layers=2)
    m = LlamaDecoder(cfg, "cuda", seed=5, weight_dtype="fp8")
    m.alloc_cache(18, 128)
    rng = np.random.default_rng(2)
    prompts = [[int(t) for t in rng.integers(5, 32000, size=int(n))] for n in rng.integers(8, 40, size=16)]
    m.ops = _Counting(m.ops)
    out = Generator(m, max_batch=16, max_seq=128, temperature=0.0, use_graphs=True).generate(prompts, 6)
    assert [len(r.tokens) for r in out] == [6] * 16 and m.ops.w8 > 0 and m.ops.dk == 0
    ref = _reference_decoder(m, 128)
    for p, r in zip(prompts, out):  # every row of the block against the fp32 reference model
        _near_argmax_under_reference(ref, p, r.tokens)


def test_fp8_decoder_with_short_k_keeps_batch1_on_bf16():
    """tiny-dec (hidden 256, FFN 512): K % 256 == 0 but K % 1024 != 0, so the fp8 copies are kept for
    gemm_dk_w8 alone (one k chunk, shorter than the prefetch ring). A batch-1 step must not send them
    to the fp8 GEMV, which refuses K = 256: it runs on the bf16 tensors, as it did before the copies
    existed. A batch-3 step streams them."""
    m = LlamaDecoder(decoder_config("tiny-dec"), "cuda", seed=7, weight_dtype="fp8")
    m.alloc_cache(16, 128)
    assert "wo_q8" in m.w["layers"][0] and not m.ops.gemv_w8_fusable(1, 256, 256, 4)
    ops = m.ops
    ref = _reference_decoder(m, 128)
    prompts = [list(range(50, 83)), list(range(300, 317)), list(range(1000, 1041))]
    for ps in (prompts[:1], prompts):
        m.ops = c = _Counting(ops)
        c.gemv = 0

        def gemm_w8(*a, _c=c, **kw):
            _c.gemv += 1
            return ops.gemm_w8(*a, **kw)
        c.gemm_w8 = gemm_w8
        out = Generator(m, max_batch=4, max_seq=128, temperature=0.0, use_graphs=False).generate(ps, 6)
        assert c.gemv == 0 and (c.w8 == 0) == (len(ps) == 1), (c.gemv, c.w8)
        for p, r in zip(ps, out):
            assert len(r.tokens) == 6
            _near_argmax_under_reference(ref, p, r.tokens)
    m.ops = ops
