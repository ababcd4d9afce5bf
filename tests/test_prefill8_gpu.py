"""fp8 (W8A8) prefill on the gfx950 kernels: rmsnorm_q8 against the two-kernel chain it replaces (bit
for bit), gemm_fp8 at the decoder's edges (ragged M and N, padded strides, the in-place residual, the
w_gu interleave), both kernels writing only their outputs, and LlamaDecoder(prefill_dtype="fp8")
against the reference ops' W8A8 model."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from docagents_amd.models import llama  # noqa: E402
from docagents_amd.models.configs import DecoderConfig  # noqa: E402
from docagents_amd.models.llama import DecodeState, LlamaDecoder, pack_prompts  # noqa: E402
from docagents_amd.ops import kernels as K  # noqa: E402
from docagents_amd.ops import reference as R  # noqa: E402

from kernel_frames import assert_frame_intact, framed, guarded  # noqa: E402

DEV = "cuda"
BF16, FP8 = torch.bfloat16, torch.float8_e4m3fn


def _rand(*shape, scale=1.0):
    return (torch.randn(*shape, device=DEV) * scale).to(BF16)


def _close(a, b, atol, rtol=0.02):
    a, b = a.float(), b.float()
    err = (a - b).abs()
    bad = (err > atol + rtol * b.abs()).sum().item()
    assert bad == 0, f"{bad} / {a.numel()} mismatches, max err {err.max().item():.4g}"


def _u8(t):
    return t.view(torch.uint8)


# ------------------------------------------------------------------------------------ rmsnorm_q8
def _norm_rows(M, D, pad):
    """x [M, D] as a view of a wider buffer (ldx = D + pad): rows over several binades, a row of zeros
    and a row whose one outlier sets the scale (every other code of that row is tiny or subnormal)."""
    torch.manual_seed(100 * M + D + pad)
    buf = _rand(M, D + pad)
    buf.mul_(torch.exp2(torch.randint(-4, 3, (M, 1), device=DEV).float()).to(BF16))
    x = buf[:, :D]
    if M >= 3:
        x[1] = 0
        x[2, D // 3] = 448.0
    else:
        x[0, D // 3] = 448.0
    return buf, x, _rand(D, scale=0.2) + 1


# 1027 rows of 3072 / 4096: the one-wave-per-row form both kernels take from 1024 rows
@pytest.mark.parametrize("M,D", [(m, d) for d in (256, 3072, 4096) for m in (1, 3, 257)] + [(1027, 3072), (1027, 4096)])
def test_rmsnorm_q8_is_bit_identical_to_the_chain(M, D):
    buf, x, g = _norm_rows(M, D, 24)
    before = buf.clone()
    hq, hs = K.quant_fp8(K.rmsnorm(x, g, 1e-5))
    q, s = K.rmsnorm_q8(x, g, 1e-5)
    assert q.dtype == FP8 and q.shape == (M, D) and s.dtype == torch.float32 and s.shape == (M,)
    assert torch.equal(s, hs) and torch.equal(_u8(q), _u8(hq))
    if M >= 3:
        assert float(s[1]) == 1.0 and not _u8(q)[1].any()  # the zero row: scale 1, codes 0
        assert float(q[2, D // 3].float().abs()) == 448.0    # the outlier is the row's largest code
    # against the fp32 oracle: the same scales up to the norm's rounding, codes within one e4m3 step
    rq, rs = R.rmsnorm_q8(x, g, 1e-5)
    assert torch.allclose(s, rs, rtol=2 ** -7)
    d = (q.float() * s[:, None] - rq.float() * rs[:, None]).abs()
    assert torch.all(d <= 0.14 * (rq.float() * rs[:, None]).abs() + 2.0 ** -8 * rs[:, None])
    # padded ldo, a longer scale buffer: the same bits, nothing else written, inputs unchanged
    obuf, oview = framed(M, D, FP8, 48, device=DEV)
    sbuf, sview = guarded(M, torch.float32, device=DEV)
    q2, s2 = K.rmsnorm_q8(x, g, 1e-5, out=oview, scale=sview)
    assert q2.data_ptr() == oview.data_ptr() and s2.data_ptr() == sview.data_ptr()
    assert torch.equal(_u8(oview), _u8(hq)) and torch.equal(sview, hs)
    assert_frame_intact(obuf, oview, "rmsnorm_q8 codes")
    assert_frame_intact(sbuf, sview, "rmsnorm_q8 scales")
    assert torch.equal(buf, before)


def test_rmsnorm_q8_row_subset_follows_the_pass():
    """route_m: rows taken out of a 1500-row pass get that pass's kernel (sum order), hence its bits."""
    M, D = 1500, 3072
    _, x, g = _norm_rows(M, D, 8)
    full_q, full_s = K.rmsnorm_q8(x, g, 1e-5)
    ix = torch.tensor([0, 2, 700, M - 1], device=DEV)
    q, s = K.rmsnorm_q8(x.index_select(0, ix), g, 1e-5, route_m=M)
    assert torch.equal(_u8(q), _u8(full_q.view(torch.uint8).index_select(0, ix))) and torch.equal(s, full_s[ix])
    hq, hs = K.quant_fp8(K.rmsnorm(x.index_select(0, ix), g, 1e-5, route_m=M))
    assert torch.equal(_u8(q), _u8(hq)) and torch.equal(s, hs)


def test_rmsnorm_q8_refuses_bad_operands():
    x, g = _rand(4, 256), _rand(256)
    with pytest.raises(ValueError):
        K.rmsnorm_q8(x[:, :252], g[:252], 1e-5)  # D % 8
    with pytest.raises(ValueError):
        K.rmsnorm_q8(x, g, 1e-5, out=torch.empty(4, 256, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        K.rmsnorm_q8(x, g, 1e-5, scale=torch.empty(3, dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError):
        K.rmsnorm_q8(x, g[:128], 1e-5)


# -------------------------------------------------------------------------------------- gemm_fp8
GEMM_SHAPES = [(1, 768, 256), (255, 320, 384), (257, 768, 3072), (513, 512, 256)]
_GEMM_CASES = {}


def _gemm_case(M, N, Kd):
    """Quantised operands of one shape, A with a padded row stride; built once, never modified."""
    key = (M, N, Kd)
    if key not in _GEMM_CASES:
        torch.manual_seed(M + N + Kd)
        x = _rand(M, Kd)
        x.mul_(torch.exp2(torch.randint(-3, 4, (M, 1), device=DEV).float()).to(BF16))  # a scale per row that matters
        w = _rand(N, Kd, scale=Kd ** -0.5)
        abuf = torch.zeros(M, Kd + 32, dtype=torch.uint8, device=DEV).view(FP8)
        aq, sa = K.quant_fp8(x, out=abuf[:, :Kd])
        wq, sw = K.quant_weight_fp8_pow2(w)  # the decoder's weight copy: a power-of-two scale per output row
        _GEMM_CASES[key] = (aq, sa, wq, sw, _rand(M, N))
    return _GEMM_CASES[key]


@pytest.mark.parametrize("M,N,Kd", GEMM_SHAPES)
@pytest.mark.parametrize("epi", [K.EPI_NONE, K.EPI_SWIGLU, K.EPI_RESID])
def test_gemm_fp8_decoder_edges(M, N, Kd, epi):
    """Against the fp32 product of the dequantised operands (the tolerance of the encoder's gemm_fp8
    test): contiguous, then into padded frames (rows >= M and columns >= N keep their canary), EPI_RESID
    out of place with another stride and in place (out is resid); inputs unchanged."""
    aq, sa, wq, sw, x0 = _gemm_case(M, N, Kd)
    assert aq.stride(0) == Kd + 32  # lda padded
    resid = x0 if epi == K.EPI_RESID else None
    nout = N // 2 if epi == K.EPI_SWIGLU else N
    keep = [_u8(aq).clone(), sa.clone(), _u8(wq).clone(), sw.clone(), x0.clone()]
    want = K.gemm_fp8(aq, sa, wq, sw, epi=epi, resid=resid)
    assert want.shape == (M, nout) and want.is_contiguous()
    _close(want, R.gemm_fp8(aq, sa, wq, sw, epi=epi, resid=resid), atol=0.03)
    for pad in (8, 24):
        buf, view = framed(M, nout, BF16, pad, device=DEV)
        if epi != K.EPI_RESID:
            got = K.gemm_fp8(aq, sa, wq, sw, epi=epi, out=view)
            assert got.data_ptr() == view.data_ptr()
        else:
            rbuf, rview = framed(M, N, BF16, pad + 32, device=DEV)  # ldr != ldc
            rview.copy_(x0)
            K.gemm_fp8(aq, sa, wq, sw, epi=epi, resid=rview, out=view)
            assert_frame_intact(rbuf, rview, "resid frame")
            assert torch.equal(rview, x0), "out-of-place resid was modified"
        assert torch.equal(view, want), f"framed out (pad {pad}) differs from the contiguous launch"
        assert_frame_intact(buf, view, f"out pad {pad}")
        if epi == K.EPI_RESID:  # the decoder's form: x += a @ w^T in place, padded ldc
            buf, view = framed(M, N, BF16, pad, device=DEV)
            view.copy_(x0)
            got = K.gemm_fp8(aq, sa, wq, sw, epi=epi, resid=view, out=view)
            assert got.data_ptr() == view.data_ptr() and torch.equal(view, want)
            assert_frame_intact(buf, view, f"in-place out pad {pad}")
    if epi == K.EPI_RESID:  # in place on a contiguous tensor
        x = x0.clone()
        assert K.gemm_fp8(aq, sa, wq, sw, epi=epi, resid=x, out=x) is x and torch.equal(x, want)
    for t, k in zip((_u8(aq), sa, _u8(wq), sw, x0), keep):
        assert torch.equal(t, k), "an input was modified"


def test_gemm_fp8_swiglu_on_the_decoder_interleave_matches_gemm():
    """w_gu as the decoder builds it (interleave_gate_up, fp8 copy): gemm_fp8's SwiGLU == the fp32
    silu(gate) * up of the separate matrices, and == gemm()'s (gemm8p) on the dequantised operands."""
    torch.manual_seed(9)
    M, F, Kd = 700, 384, 512
    gate, up = _rand(F, Kd, scale=Kd ** -0.5), _rand(F, Kd, scale=Kd ** -0.5)
    wq, sw = K.quant_weight_fp8_pow2(R.interleave_gate_up(gate, up))
    w = (wq.float() * sw[:, None]).to(BF16)  # exact
    gq, gs = K.quant_weight_fp8_pow2(gate)
    uq, us = K.quant_weight_fp8_pow2(up)
    aq, sa = K.quant_fp8(_rand(M, Kd))
    a = (aq.float() * sa[:, None])
    got = K.gemm_fp8(aq, sa, wq, sw, epi=K.EPI_SWIGLU)
    ref = (torch.nn.functional.silu(a @ (gq.float() * gs[:, None]).t()) * (a @ (uq.float() * us[:, None]).t()))
    _close(got, ref.to(BF16), atol=0.03)
    # the bf16 kernel on (a rounded to bf16, w): the same layout, up to the activations' bf16 rounding
    _close(got, K.gemm(a.to(BF16), w, epi=K.EPI_SWIGLU), atol=0.03)


def test_gemm_fp8_rows_do_not_depend_on_m():
    """A row subset of a 700-row product has the full launch's bits (the tail cut's premise)."""
    aq, sa, wq, sw, _ = _gemm_case(513, 512, 256)
    full = K.gemm_fp8(aq, sa, wq, sw)
    ix = torch.tensor([0, 255, 256, 512], device=DEV)
    sub = K.gemm_fp8(_u8(aq).index_select(0, ix).view(FP8), sa[ix].contiguous(), wq, sw)
    assert torch.equal(sub, full.index_select(0, ix))


def test_gemm_fp8_refuses_bad_operands():
    aq, sa, wq, sw, x0 = _gemm_case(255, 320, 384)
    with pytest.raises(ValueError):
        K.gemm_fp8(aq, sa, wq, sw, epi=K.EPI_RESID)  # no resid
    with pytest.raises(ValueError):
        K.gemm_fp8(aq, sa, wq, sw, epi=K.EPI_RESID, resid=x0[:, :312], out=x0[:, :312])
    big = torch.zeros(256, 328, dtype=BF16, device=DEV)
    with pytest.raises(ValueError):  # overlapping, but not the same rows
        K.gemm_fp8(aq, sa, wq, sw, epi=K.EPI_RESID, resid=big[:255, :320], out=big[1:, :320])
    with pytest.raises(ValueError):
        K.gemm_fp8(aq, sa, wq[:312], sw[:312], epi=K.EPI_SWIGLU)  # N % 32
    with pytest.raises(ValueError):
        K.gemm_fp8(aq, sa[:100], wq, sw)


# ----------------------------------------------------------------------------------------- model
SMALL = DecoderConfig("small-w8a8", vocab=512, hidden=256, layers=2, heads=4, kv_heads=4, ffn=512, max_pos=1024,
                      rope_theta=10000.0)
LENS = (130, 61, 1, 77)  # 269 rows: two 256-row tiles, the second one ragged


@pytest.fixture(scope="module")
def weights():
    return LlamaDecoder(SMALL, DEV, seed=0, weight_dtype="fp8", prefill_dtype="fp8").w


def _models(weights, kv):
    m = LlamaDecoder(SMALL, DEV, weights=weights, weight_dtype="fp8", prefill_dtype="fp8", kv_dtype=kv)
    r = LlamaDecoder(SMALL, DEV, weights=weights, weight_dtype="fp8", prefill_dtype="fp8", kv_dtype=kv)
    r.ops = R  # the W8A8 emulation: dequantise both sides, fp32 product, the same roundings
    return m, r


def _to(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _prefill(m, P=0):
    """One packed prefill of LENS (after a shared head of P tokens in slot 0) -> (logits, decode state)."""
    rng = np.random.default_rng(3)
    head = [int(t) for t in rng.integers(1, SMALL.vocab, size=P)]
    prompts = [[int(t) for t in rng.integers(1, SMALL.vocab, size=n)] for n in LENS]
    n = len(LENS)
    m.alloc_cache(n + 1, 512)
    prefix = None
    if P:
        m.prefill(_to(np.asarray(head, dtype=np.int32)), _to(np.arange(P, dtype=np.int32)),
                  _to(np.zeros(P, dtype=np.int32)), _to(np.array([0, P], dtype=np.int32)), P,
                  _to(np.array([P - 1], dtype=np.int64)))
        prefix = (0, P)
    flat, pos, cu, lens = pack_prompts(prompts)
    slot_tok = np.repeat(np.arange(1, n + 1, dtype=np.int32), lens)
    logits = m.prefill(_to(flat), _to(pos + P), _to(slot_tok), _to(cu), int(lens.max()),
                       _to((cu[1:] - 1).astype(np.int64)), prefix=prefix)
    st = DecodeState(m, n, 4, 0.0, 0)
    plen = _to((lens + P).astype(np.int32))
    st.pos.copy_(plen - 1); st.lens.copy_(plen); st.slot.copy_(torch.arange(1, n + 1, dtype=torch.int32))
    st.active.fill_(1); st.start.copy_(plen - 1)
    if P:
        st.pre.copy_(torch.tensor([[P, 0]] * n, dtype=torch.int32))
    # greedy first token: advances pos / lens to the new token's position, as the generator does
    m.sample(logits, 0.0, 0, 0, out_tok=st.tokens, out_lp=st.lp, conf=st.conf, active=st.active, ctr=st.pos,
             pos=st.pos, lens=st.lens, hist=st.hist, start=st.start, eos=())
    torch.cuda.synchronize()
    return logits.clone(), st


@pytest.mark.parametrize("kv", ["bf16", "fp8"])
@pytest.mark.parametrize("P", [0, 192])
def test_decoder_fp8_prefill_matches_the_w8a8_reference(weights, kv, P):
    """GPU kernels against the reference ops on the same W8A8 model, at the tolerance
    tests/test_models_gpu.py allows the bf16 decoder against its reference (0.05 on the logits); then
    one decode step from the cache this prefill wrote, both arms fed the same token."""
    m, r = _models(weights, kv)
    assert m._pf8_layer(sum(LENS)) and (P == 0 or m._pf8_layer(P))
    lg, st = _prefill(m, P)
    lr, sr = _prefill(r, P)
    assert torch.isfinite(lg.float()).all()
    assert (lg.float() - lr.float()).abs().max() < 0.05
    if kv == "bf16":
        # every cached row is where the reference put it (the numbers are checked through the logits:
        # quant_fp8 and its oracle may round an element to neighbouring codes, x * (1 / s) against x / s,
        # which moves single K / V elements by more than a bf16 tolerance; a misplaced or missing row
        # is off by its whole norm)
        got, ref = m.cache.buf.float(), r.cache.buf.float()
        written = ref.abs().amax(-1) > 0
        assert torch.equal(written, got.abs().amax(-1) > 0)
        assert torch.all((got - ref).norm(dim=-1)[written] < 0.25 * ref.norm(dim=-1)[written])
    assert torch.equal(st.pos, sr.pos) and torch.equal(st.lens, sr.lens)
    st.tokens.copy_(sr.tokens)  # one history in both arms, whatever a near-tie did to the first token
    m.decode_step(st)
    r.decode_step(sr)
    torch.cuda.synchronize()
    assert torch.isfinite(st.logits.float()).all()
    assert (st.logits.float() - sr.logits.float()).abs().max() < 0.05


def test_decoder_fp8_prefill_differs_from_bf16_prefill(weights):
    """The option changes the prefill (the fp8 path is taken on the GPU), within the CPU test's bound."""
    m, _ = _models(weights, "bf16")
    b = LlamaDecoder(SMALL, DEV, weights=weights, weight_dtype="fp8")
    lm, _ = _prefill(m)
    lb, _ = _prefill(b)
    assert not torch.equal(lm, lb)
    rel = float((lm.float() - lb.float()).norm() / lb.float().norm())
    assert 0.0 < rel <= 8 * 2 ** -4 / 3 ** 0.5, rel


@pytest.mark.parametrize("kv", ["bf16", "fp8"])
def test_decoder_fp8_prefill_tail_cut_is_bit_identical(weights, kv, monkeypatch):
    m, _ = _models(weights, kv)
    out = {}
    for tail in (True, False):
        monkeypatch.setattr(llama, "_PREFILL_TAIL", tail)
        assert (m._tail_routes(sum(LENS)) is not None) == tail
        lg, _ = _prefill(m, 192)
        cache = m.cache.buf if kv == "bf16" else m.cache.codes.view(torch.uint8)
        out[tail] = (lg, cache.clone())
    assert torch.equal(out[True][0], out[False][0])
    assert torch.equal(out[True][1], out[False][1])


def test_engine_fp8_prefill_answers_and_summarises():
    from docagents_amd.engine.engine import Engine
    eng = Engine("tiny-enc", "tiny-dec", DEV, max_batch=4, max_seq=1024, max_new_tokens=8, summary_max_new=8,
                 load_encoder=False, llm_weight_dtype="fp8", llm_prefill_dtype="fp8")
    assert eng.decoder.prefill_dtype == "fp8"
    calls = {"n": 0}
    real = K.gemm_fp8

    def counted(*a, **kw):
        calls["n"] += 1
        return real(*a, **kw)
    eng.decoder.ops = type("Ops", (), {"__getattr__": lambda self, k: counted if k == "gemm_fp8" else getattr(K, k)})()
    ans = eng.answer_many([("What memory?", [eng._ids("The MI355X has 288 GB of HBM3E. " * 30)], 0.9)], 8)
    assert len(ans) == 1 and isinstance(ans[0][0], str) and 0.0 <= ans[0][1] <= 1.0
    assert calls["n"] > 0  # a prompt of more than 128 tokens: the fp8 products ran
    summ = eng.summarize_many(["word " * 300])
    assert len(summ) == 1
    torch.cuda.synchronize()
    assert any(st.graph is not None for st in eng.gen.states.values())  # decode graphs captured as before
