"""fp8 (W8A8) prefill of the decoder on the CPU (reference ops): the LLM_PREFILL_DTYPE startup checks,
the prefill_w8_fusable truth table, the fp32 oracle of rmsnorm_q8, and a small decoder whose fp8
prefill is compared with the bf16 prefill of the same fp8-weight model."""
import numpy as np
import pytest
import torch

from docagents_amd import config
from docagents_amd.models.configs import DecoderConfig
from docagents_amd.models.llama import LlamaDecoder, TPContext, pack_prompts
from docagents_amd.ops import gemm_plan as G
from docagents_amd.ops import reference as R

# every product of this decoder is on the fp8 route: K = 256 / 512 (% 128), N = 768 / 256 / 1024 / 256
SMALL = DecoderConfig("small-w8a8", vocab=512, hidden=256, layers=2, heads=4, kv_heads=4, ffn=512, max_pos=1024,
                      rope_theta=10000.0)
LENS = (130, 61, 1, 77)  # 269 rows: above the decode range, two row tiles of 256
PRODUCTS = (("wqkv", G.EPI_NONE), ("wo", G.EPI_RESID), ("w_gu", G.EPI_SWIGLU), ("w_down", G.EPI_RESID))


def test_config_key_and_startup_checks():
    assert config.load({}).validate_engine().llm_prefill_dtype == "bf16"
    assert config.Config.LLM_PREFILL_DTYPES == ("bf16", "fp8")
    ok = config.load({"LLM_PREFILL_DTYPE": "fp8", "LLM_WEIGHT_DTYPE": "fp8"}).validate_engine()
    assert ok.llm_prefill_dtype == "fp8" and ok.llm_weight_dtype == "fp8"
    with pytest.raises(ValueError, match="LLM_PREFILL_DTYPE"):
        config.load({"LLM_PREFILL_DTYPE": "fp8"}).validate_engine()  # no fp8 weight copy
    with pytest.raises(ValueError, match="LLM_PREFILL_DTYPE"):
        config.load({"LLM_PREFILL_DTYPE": "fp8", "LLM_WEIGHT_DTYPE": "fp8", "TP_SIZE": "2"}).validate_engine()
    with pytest.raises(ValueError, match="LLM_PREFILL_DTYPE"):
        config.load({"LLM_PREFILL_DTYPE": "int8", "LLM_WEIGHT_DTYPE": "fp8"}).validate_engine()


def test_decoder_option_checks():
    with pytest.raises(ValueError, match="prefill_dtype"):
        LlamaDecoder(SMALL, "cpu", prefill_dtype="fp8", weight_dtype="bf16")
    with pytest.raises(ValueError, match="prefill_dtype"):
        LlamaDecoder(SMALL, "cpu", prefill_dtype="int8", weight_dtype="fp8")
    with pytest.raises(ValueError, match="TP"):
        LlamaDecoder(SMALL, "cpu", tp=TPContext(0, 2), prefill_dtype="fp8", weight_dtype="fp8")
    assert LlamaDecoder(SMALL, "cpu").prefill_dtype == "bf16"


def test_prefill_w8_fusable_truth_table():
    f = G.prefill_w8_fusable
    for M in (1, 2, 32, 64, 128):  # a decode step's rows keep their routes
        assert not f(M, 9216, 3072)
    assert f(129, 9216, 3072) and f(2930, 9216, 3072)
    assert not f(4096, 9216, 192)  # K is no whole 128-code MFMA step
    assert not f(4096, 9216, 64)
    assert not f(4096, 9220, 3072)  # N % 8
    assert f(4096, 16, 3072, G.EPI_NONE) and not f(4096, 16, 3072, G.EPI_SWIGLU)  # SwiGLU: N % 32
    assert f(4096, 32, 3072, G.EPI_SWIGLU)
    assert not f(4096, 3072, 3072, G.EPI_BIAS) and not f(4096, 3072, 3072, G.EPI_GELU)
    phi3 = ((9216, 3072, G.EPI_NONE), (3072, 3072, G.EPI_RESID), (16384, 3072, G.EPI_SWIGLU),
            (3072, 8192, G.EPI_RESID))
    llama8b = ((6144, 4096, G.EPI_NONE), (4096, 4096, G.EPI_RESID), (28672, 4096, G.EPI_SWIGLU),
               (4096, 14336, G.EPI_RESID))
    # the one measured loss (profiles/prefill8/README.md): Phi-3's O projection in a batch-1 prefill, a residual
    # product whose 144 tiles leave the chip under-filled on a K of 3072; the down projection (K = 8192) won there
    held_back = {(2930, 3072, 3072, G.EPI_RESID)}
    for N, K, epi in phi3 + llama8b:
        for M in (2930, 29440, 32768):
            assert f(M, N, K, epi) == ((M, N, K, epi) not in held_back), (M, N, K, epi)
    assert f(2930, 3072, 3072, G.EPI_NONE) and f(600, 3072, 3072, G.EPI_RESID) and f(5377, 3072, 3072, G.EPI_RESID)
    assert not f(5376, 3072, 3072, G.EPI_RESID) and f(5376, 3072, 3200, G.EPI_RESID)
    assert R.prefill_w8_fusable(2930, 9216, 3072) and not R.prefill_w8_fusable(128, 9216, 3072)


def test_rmsnorm_q8_oracle_is_the_quantised_norm():
    torch.manual_seed(0)
    x = torch.randn(5, 256).to(torch.bfloat16)
    x[2] = 0
    g = (torch.randn(256) * 0.1 + 1).to(torch.bfloat16)
    q, s = R.rmsnorm_q8(x, g, 1e-5)
    h = R.rmsnorm(x, g, 1e-5)
    rq, rs = R.quant_fp8(h)
    assert q.dtype == torch.float8_e4m3fn and s.dtype == torch.float32 and s.shape == (5,)
    assert torch.equal(q.view(torch.uint8), rq.view(torch.uint8)) and torch.equal(s, rs)
    assert float(s[2]) == 1.0 and not q[2].float().any()  # an all-zero row: scale 1, codes 0
    assert torch.allclose(q.float() * s[:, None], h.float(), rtol=2 ** -4, atol=1e-3)
    out, sc = torch.empty(5, 256, dtype=torch.float8_e4m3fn), torch.empty(8)
    q2, s2 = R.rmsnorm_q8(x, g, 1e-5, out=out, scale=sc)
    assert q2 is out and torch.equal(out.view(torch.uint8), q.view(torch.uint8)) and torch.equal(sc[:5], s)


def test_reference_gemm_fp8_adds_in_place():
    torch.manual_seed(1)
    a, w = torch.randn(7, 128).to(torch.bfloat16), (torch.randn(16, 128) * 0.1).to(torch.bfloat16)
    aq, sa = R.quant_fp8(a)
    wq, sw = R.quant_weight_fp8_pow2(w)
    x = torch.randn(7, 16).to(torch.bfloat16)
    want = R.gemm_fp8(aq, sa, wq, sw, epi=G.EPI_RESID, resid=x.clone())
    got = R.gemm_fp8(aq, sa, wq, sw, epi=G.EPI_RESID, resid=x, out=x)
    assert got is x and torch.equal(x, want)


class _Counting:
    """The ops module with a call counter per op."""

    def __init__(self, ops):
        self._ops, self.calls = ops, {}

    def __getattr__(self, name):
        f = getattr(self._ops, name)
        if not callable(f):
            return f

        def g(*a, **kw):
            self.calls[name] = self.calls.get(name, 0) + 1
            return f(*a, **kw)
        return g


def _prefill(m, lens=LENS, seed=3):
    rng = np.random.default_rng(seed)
    prompts = [[int(t) for t in rng.integers(1, m.cfg.vocab, size=n)] for n in lens]
    flat, pos, cu, ln = pack_prompts(prompts)
    m.alloc_cache(len(lens), 256)
    slot_tok = np.repeat(np.arange(len(lens), dtype=np.int32), ln)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    return m.prefill(to(flat), to(pos), to(slot_tok), to(cu), int(ln.max()), to((cu[1:] - 1).astype(np.int64)))


@pytest.fixture(scope="module")
def pair():
    b = LlamaDecoder(SMALL, "cpu", seed=0, weight_dtype="fp8")
    m = LlamaDecoder(SMALL, "cpu", seed=0, weight_dtype="fp8", prefill_dtype="fp8")
    return b, m


def test_fp8_copy_kept_for_every_prefill_product(pair):
    b, m = pair
    for L in m.w["layers"]:
        for k, _ in PRODUCTS:
            q, s, w = L[k + "_q8"], L[k + "_s8"], L[k]
            assert q.dtype == torch.float8_e4m3fn and q.shape == w.shape and s.shape == (w.shape[0],)
            assert torch.equal((q.float() * s[:, None]).to(torch.bfloat16), w)  # the bf16 tensor IS the copy
    # the same model in both arms, and no copy in the bf16-prefill arm where no decode kernel takes one (K = 256 / 512
    # is no GEMV shape; gemm_dk_w8 takes them all here, so compare the tensors only)
    for Lb, Lm in zip(b.w["layers"], m.w["layers"]):
        for k, _ in PRODUCTS:
            assert torch.equal(Lb[k], Lm[k])
    k64 = DecoderConfig("k64", vocab=64, hidden=64, layers=1, heads=1, kv_heads=1, ffn=64, max_pos=64, rope_theta=1e4)
    r = LlamaDecoder(k64, "cpu", seed=0, weight_dtype="fp8", prefill_dtype="fp8")
    assert not any(k.endswith("_q8") for k in r.w["layers"][0])  # K = 64: the route refuses every product
    assert not r._pf8_layer(4096)


def test_fp8_prefill_is_taken_and_stays_within_the_e4m3_bound(pair):
    """fp8 prefill against bf16 prefill of the same fp8-weight model, 269 rows, reference ops.

    The bound. A product's input row is stored as e4m3 codes times one row scale: 3 mantissa bits, so
    round-to-nearest moves an element by at most u = 2^-4 of itself (codes below 2^-6 are subnormal
    and move by at most 2^-10 of the row's code range, which is nothing next to the row's norm).
    Rounding errors of different elements are independent and spread evenly over +-u, so their rms is
    u / sqrt(3), and a product y_j = sum_i w_ji x_i (1 + d_i) with such d_i carries an rms error of
    u / sqrt(3) times sqrt(sum_i w_ji^2 x_i^2): relative to the output's own rms, e1 = u / sqrt(3) =
    0.0361 wherever the terms of the sum add like independent ones, as they do for random weights.
    RMSNorm and the LM head keep a relative error as it is, the residual adds and the attention
    average do not enlarge it, and the embedding rows at the bottom of the residual stream carry
    none. The P = 4 * layers = 8 products each put e1 into the stream; if every one of them pushed
    the logits the same way the errors would add up, so

        ||logits_fp8 - logits_bf16||_2 / ||logits_bf16||_2  <=  P * u / sqrt(3)  =  8 * 2^-4 / sqrt(3)  =  0.289,

    with sqrt(P) * e1 = 0.10 the size to expect from independent contributions. The weights' own
    quantisation is in both arms and cancels. The bound was fixed before the first run."""
    b, m = pair
    m.ops = _Counting(R)
    try:
        lm = _prefill(m)
        calls = dict(m.ops.calls)
    finally:
        m.ops = R
    lb = _prefill(b)
    n = SMALL.layers
    assert calls["gemm_fp8"] == 4 * n and calls["rmsnorm_q8"] == 2 * n and calls["quant_fp8"] == 2 * n, calls
    assert calls.get("gemm_rope", 0) == 0 and calls["rope_cache"] == n, calls
    assert lm.shape == lb.shape == (len(LENS), SMALL.vocab) and torch.isfinite(lm.float()).all()
    assert not torch.equal(lm, lb)  # the path is really taken
    rel = float((lm.float() - lb.float()).norm() / lb.float().norm())
    print(f"fp8 prefill vs bf16 prefill (reference ops): relative L2 logit error {rel:.4f}, "
          f"max |dlogit| {float((lm.float() - lb.float()).abs().max()):.4f}")
    assert 0.0 < rel <= 8 * 2 ** -4 / 3 ** 0.5, rel
    # the keys / values the prefill cached moved by the QKV products' input rounding only
    assert not torch.equal(m.cache.buf, b.cache.buf)
    assert float((m.cache.buf.float() - b.cache.buf.float()).norm() / b.cache.buf.float().norm()) <= 8 * 2 ** -4 / 3 ** 0.5


def test_decode_rows_and_refused_shapes_stay_on_the_bf16_prefill(pair):
    """A prefill of at most 128 rows is the bf16 prefill, bit for bit and launch for launch."""
    b, m = pair
    m.ops = _Counting(R)
    try:
        lm = _prefill(m, lens=(60, 40))
        calls = dict(m.ops.calls)
    finally:
        m.ops = R
    assert "gemm_fp8" not in calls and "rmsnorm_q8" not in calls, calls
    assert torch.equal(lm, _prefill(b, lens=(60, 40)))


def test_tail_cut_keeps_the_full_pass_bits(pair, monkeypatch):
    from docagents_amd.models import llama
    _, m = pair
    monkeypatch.setattr(llama, "_PREFILL_TAIL", True)
    on = _prefill(m).clone()
    monkeypatch.setattr(llama, "_PREFILL_TAIL", False)
    off = _prefill(m).clone()
    assert torch.equal(on, off)


def test_engine_passes_the_option_through():
    from docagents_amd.engine.engine import Engine
    kw = dict(max_batch=2, max_seq=256, max_new_tokens=2, use_graphs=False, load_encoder=False)
    e = Engine("tiny-enc", "tiny-dec", "cpu", llm_weight_dtype="fp8", llm_prefill_dtype="fp8", **kw)
    assert e.decoder.prefill_dtype == "fp8" and "wo_q8" in e.decoder.w["layers"][0]
    assert Engine("tiny-enc", "tiny-dec", "cpu", **kw).decoder.prefill_dtype == "bf16"
    with pytest.raises(ValueError, match="prefill_dtype"):
        Engine("tiny-enc", "tiny-dec", "cpu", llm_prefill_dtype="fp8", **kw)
