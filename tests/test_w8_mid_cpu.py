"""The 33..128-row fp8 decode route on the CPU: the planner's predicate and plans (ops/gemm_plan.py
tile_w8_fusable, plan_tile_w8 / plan_dk_splitk_w8 / plan_resid_norm_w8: the bf16 plan's tile, split
count and workspace), the reference ops (the bf16 form's reference op on the dequantised matrix), and
the CPU decoder with weight_dtype="fp8" running a 40-row step through them."""
import copy

import pytest
import torch

from docagents_amd.engine.generator import Generator
from docagents_amd.models.configs import decoder_config
from docagents_amd.models.llama import LlamaDecoder
from docagents_amd.ops import gemm_plan as P
from docagents_amd.ops import kernels as K
from docagents_amd.ops import reference as R

NEW_OPS = ("gemm_tile_w8", "gemm_dk_splitk_w8", "gemm_resid_norm_w8")


def test_tile_w8_fusable_truth_table():
    for mod in (P, K, R):
        f = mod.tile_w8_fusable
        assert not f(32, 128, 256) and f(33, 128, 256) and f(128, 128, 256) and not f(129, 128, 256)
        assert not f(1, 128, 256) and not f(2, 128, 256)
        assert f(64, 128, 128) and f(64, 128, 192) and not f(64, 128, 96) and not f(64, 128, 0)
        assert not f(64, 128, 64)  # one k-tile: the kernels take it, the route holds it back
        assert f(64, 72, 256) and not f(64, 76, 256)
        assert not f(64, 48, 256, P.EPI_SWIGLU) and f(64, 64, 256, P.EPI_SWIGLU) and f(64, 48, 256, P.EPI_RESID)
        assert f(64, 64, 256, P.EPI_BIAS) and not f(64, 64, 256, P.EPI_GELU)
    # held back from the A/B: 65..96 rows, the 128x64 tile (N < 8192), K <= 3072
    assert not P.tile_w8_fusable(96, 3072, 3072, P.EPI_RESID) and not P.tile_w8_fusable(65, 3072, 3072, P.EPI_RESID)
    assert P.tile_w8_fusable(97, 3072, 3072, P.EPI_RESID) and P.tile_w8_fusable(64, 3072, 3072, P.EPI_RESID)
    assert P.tile_w8_fusable(96, 3072, 8192, P.EPI_RESID) and P.tile_w8_fusable(96, 9216, 3072)
    # the neighbours keep their rules
    assert P.DK_W8_MAX_M == 32 and not P.dk_w8_fusable(33, 64, 512) and P.dk_w8_fusable(32, 64, 512)


def _products(name):
    c = decoder_config(name)
    qkv = (c.heads + 2 * c.kv_heads) * c.head_dim
    return [(qkv, c.hidden, P.EPI_NONE), (c.hidden, c.heads * c.head_dim, P.EPI_RESID),
            (2 * c.ffn, c.hidden, P.EPI_SWIGLU), (c.hidden, c.ffn, P.EPI_RESID), (c.vocab, c.hidden, P.EPI_NONE)]


@pytest.mark.parametrize("model", ["phi3-mini", "llama3-8b"])
@pytest.mark.parametrize("M", [40, 64, 100, 128])
def test_plans_are_the_bf16_plans(model, M):
    """The fp8 launch and the bf16 launch of a product must agree on tile, split count and workspace,
    or bit-identity is lost: every plan is derived from the bf16 one."""
    for N, Kd, epi in _products(model):
        assert P.tile_w8_fusable(M, N, Kd, epi)
        b = P.plan(M, N, Kd, epi, cus=256)
        t = P.plan_tile_w8(M, N, Kd, epi, cus=256)
        if b.family == "dk_splitk":  # gemm() hands 33..64 rows to da_gemm_dk_splitk: 64x128 tiles at dk_splits
            assert M <= 64 and t == P.GemmPlan("tile", P.TILE_64x128, P.dk_splits(N, Kd), b.ws_bytes)
            assert b.ws_bytes == b.splits * M * N * 4 and b.splits == P.dk_splits(N, Kd)
        else:
            assert t == b and t.tile in (P.TILE_64x128, P.TILE_128x64_PF4)
        if M <= 64:
            for ssq in (False, True):
                if ssq and N % 512:
                    with pytest.raises(ValueError):
                        P.plan_dk_splitk_w8(M, N, Kd, ssq)
                else:
                    assert P.plan_dk_splitk_w8(M, N, Kd, ssq) == P.plan_dk(M, N, Kd, ssq)
                    assert P.plan_dk(M, N, Kd, ssq).family == "dk_splitk"
        else:
            with pytest.raises(ValueError):
                P.plan_dk_splitk_w8(M, N, Kd)
        if epi == P.EPI_RESID:
            r = P.plan_resid_norm_w8(M, N, Kd)
            assert r == P.plan_resid_norm(M, N, Kd) and r.tile == (P.TILE_64x128 if M <= 64 else P.TILE_128x64_PF4)
            assert r.ws_bytes == r.splits * M * N * 4


def test_plans_refuse_a_tile_without_an_fp8_form():
    with pytest.raises(ValueError):
        P.plan_resid_norm_w8(32, 3072, 3072)  # the 32x128 tile
    with pytest.raises(ValueError):
        P.plan_tile_w8(16, 3072, 64, cus=256)
    with pytest.raises(ValueError):
        P.plan_dk_splitk_w8(32, 3072, 3072)


def test_reference_ops_equal_the_bf16_reference_ops_on_the_dequantised_weights():
    g = torch.Generator().manual_seed(5)
    M, N, Kd = 40, 512, 256
    a = torch.randn(M, Kd, generator=g).to(torch.bfloat16)
    w = torch.randn(N, Kd, generator=g) * Kd ** -0.5 * torch.exp2(torch.randint(-6, 7, (N, 1), generator=g).float())
    q, s = R.quant_weight_fp8_pow2(w.to(torch.bfloat16))
    dq = (q.float() * s[:, None]).to(torch.bfloat16)
    assert torch.equal(dq.float(), q.float() * s[:, None]) and len(set(s.tolist())) > 4
    bias = torch.randn(N, generator=g).to(torch.bfloat16)
    resid = torch.randn(M, N, generator=g).to(torch.bfloat16)
    gamma = torch.rand(N, generator=g).to(torch.bfloat16)
    ssq = torch.rand(4 * 64, generator=g) * Kd
    for epi, kw in ((R.EPI_NONE, {}), (R.EPI_BIAS, {"bias": bias}), (R.EPI_SWIGLU, {}), (R.EPI_RESID, {"resid": resid})):
        assert torch.equal(R.gemm_tile_w8(a, q, s, epi=epi, **kw), R.gemm(a, dq, epi=epi, **kw))
        for norm in (None, (ssq, 4, 1e-5)):
            if norm is not None and epi == R.EPI_RESID:
                continue
            assert torch.equal(R.gemm_dk_splitk_w8(a, q, s, epi=epi, norm_in=norm, **kw),
                               R.gemm_dk(a, dq, epi=epi, norm_in=norm, **kw))
    parts = R.dk_parts(N, M)
    assert parts == N // 512
    so8, so = torch.zeros(parts * 64), torch.zeros(parts * 64)
    y8 = R.gemm_dk_splitk_w8(a, q, s, epi=R.EPI_RESID, resid=resid, ssq_out=so8)
    y = R.gemm_dk(a, dq, epi=R.EPI_RESID, resid=resid, ssq_out=so)
    assert torch.equal(y8, y) and torch.equal(so8, so) and float(so8.view(parts, 64)[:, :M].sum()) > 0
    x8, x = resid.clone(), resid.clone()
    h8 = R.gemm_resid_norm_w8(a, q, s, x8, gamma, 1e-5, out=x8)
    h = R.gemm_resid_norm(a, dq, x, gamma, 1e-5, out=x)
    assert torch.equal(h8, h) and torch.equal(x8, x) and not torch.equal(x, resid)


class _Counting:
    """``ops`` with the calls of the new ops, gemm_dk_w8, gemm_dk and gemm counted per op and row count."""

    def __init__(self, ops):
        self._ops, self.calls = ops, {}

    def __getattr__(self, name):
        fn = getattr(self._ops, name)
        if name not in NEW_OPS + ("gemm_dk_w8", "gemm_dk", "gemm", "gemm_resid_norm"):
            return fn

        def counted(a, *args, **kw):
            self.calls[(name, a.shape[0])] = self.calls.get((name, a.shape[0]), 0) + 1
            return fn(a, *args, **kw)
        return counted

    def n(self, names, rows):
        return sum(v for (nm, r), v in self.calls.items() if nm in names and r == rows)


def test_cpu_decoder_fp8_40_rows_runs_the_new_ops_and_generates_the_bf16_tokens():
    """tiny-dec (hidden 256): a 40-row step is a gemm_dk-structured step; QKV, gate/up and the LM head go
    to gemm_dk_splitk_w8, O and down (row sums with 256 % 512 != 0: the dk kernel's own part layout)
    stay on the bf16 gemm_dk. The bf16 decoder on the dequantised weights never calls a new op."""
    cfg = decoder_config("tiny-dec")
    m = LlamaDecoder(cfg, "cpu", seed=3, weight_dtype="fp8")
    m.alloc_cache(41, 64)
    b = LlamaDecoder(cfg, "cpu", weights=copy.deepcopy(m.w))
    b.alloc_cache(41, 64)
    m.ops, b.ops = _Counting(m.ops), _Counting(b.ops)
    prompts = [list(range(40 + 3 * i, 47 + 3 * i + i % 5)) for i in range(40)]
    new = 3
    got = Generator(m, max_batch=40, max_seq=64, temperature=0.0, use_graphs=False).generate(prompts, new)
    want = Generator(b, max_batch=40, max_seq=64, temperature=0.0, use_graphs=False).generate(prompts, new)
    assert [len(r.tokens) for r in got] == [new] * 40
    steps = new - 1
    assert m.ops.n(("gemm_dk_splitk_w8",), 40) == steps * (2 * cfg.layers + 1), m.ops.calls
    assert m.ops.n(("gemm_dk",), 40) == steps * 2 * cfg.layers and m.ops.n(("gemm_dk_w8",), 40) == 0
    assert b.ops.n(NEW_OPS + ("gemm_dk_w8",), 40) == 0 and b.ops.n(("gemm_dk",), 40) == steps * (4 * cfg.layers + 1)
    assert [r.tokens for r in got] == [r.tokens for r in want]


def test_cpu_decoder_fp8_fused_norm_body_runs_tile_and_resid_norm_ops(monkeypatch):
    """The fused-norm body (what 65..128 rows run; forced here at 40 rows by switching the gemm_dk body
    off) sends QKV, gate/up and the LM head to gemm_tile_w8 and O and down to gemm_resid_norm_w8, with
    the bf16 decoder's tokens."""
    cfg = decoder_config("tiny-dec")
    m = LlamaDecoder(cfg, "cpu", seed=4, weight_dtype="fp8")
    m.alloc_cache(41, 64)
    b = LlamaDecoder(cfg, "cpu", weights=copy.deepcopy(m.w))
    b.alloc_cache(41, 64)
    monkeypatch.setattr(LlamaDecoder, "_dk_decode", lambda self, B: False)
    m.ops, b.ops = _Counting(m.ops), _Counting(b.ops)
    prompts = [list(range(30 + 2 * i, 38 + 2 * i + i % 3)) for i in range(40)]
    got = Generator(m, max_batch=40, max_seq=64, temperature=0.0, use_graphs=False).generate(prompts, 2)
    want = Generator(b, max_batch=40, max_seq=64, temperature=0.0, use_graphs=False).generate(prompts, 2)
    assert m.ops.n(("gemm_tile_w8",), 40) == 2 * cfg.layers + 1, m.ops.calls
    assert m.ops.n(("gemm_resid_norm_w8",), 40) == 2 * cfg.layers
    # the prefill's 40 last-token rows run gemm() in both arms; the decode step's products only in the bf16 arm
    bf = ("gemm", "gemm_resid_norm")
    assert b.ops.n(NEW_OPS, 40) == 0 and b.ops.n(bf, 40) - m.ops.n(bf, 40) == 4 * cfg.layers + 1
    assert [r.tokens for r in got] == [r.tokens for r in want]


def test_fp8_copy_kept_for_a_weight_only_the_new_predicate_accepts():
    """A weight neither the fp8 GEMV (K % 1024) nor gemm_dk_w8 (K % 256, N % 16) takes keeps its copy
    for the 33..128-row ops; the embedding and the norms never get one."""
    assert P.tile_w8_fusable(64, 3080, 192) and not P.dk_w8_fusable(2, 3080, 192) and not P.gemv_w8_fusable(1, 3080, 192)
    m = LlamaDecoder(decoder_config("tiny-dec"), "cpu", seed=3, weight_dtype="fp8")
    L = m.w["layers"][0]
    assert all(k + "_q8" in L for k in ("wqkv", "wo", "w_gu", "w_down")) and "lm_head_q8" in m.w
    assert "embed_q8" not in m.w and "norm_q8" not in m.w and "ln_attn_q8" not in L and "ln_mlp_q8" not in L


def test_engine_fp8_still_builds_on_cpu():
    from docagents_amd.engine.engine import Engine
    e = Engine("tiny-enc", "tiny-dec-tp8", "cpu", max_batch=2, max_seq=512, max_new_tokens=4, summary_max_new=4,
               temperature=0.0, use_graphs=False, load_encoder=False, llm_weight_dtype="fp8")
    assert e.decoder.weight_dtype == "fp8" and "wqkv_q8" in e.decoder.w["layers"][0]
    text, conf = e.answer_text("what is this?", "some context words", 0.5)
    assert isinstance(text, str) and 0.0 <= conf <= 1.0
