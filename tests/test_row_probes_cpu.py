"""The row-kernel criteria of tests/row_probes.py bite: a plain torch model with the kernels' structure
(thread t owns the 8-element chunks t + i * row_threads(D), i < MAXCH; per-wave then per-block sums;
the one-wave-per-row form) passes every criterion at every width the GPU file launches, and each
one-element mutant of that model fails. check_reference() holds for every GPU case. No GPU needed.

The negative control runs the same mutants under the old criteria (_close(atol=0.02..0.03,
rtol=0.02) and friends on test_kernels_gpu.py's Gaussian inputs): see
test_old_criteria_on_gaussian_inputs for what it showed."""
import pytest
import torch

import row_probes as P
from row_probes import BF16, F16, FP8, MAXCH

GPU_WIDTHS = sorted({8, *P.WIDTHS, *P.ROWS_WIDTHS, *P.F16_WIDTHS})
MUTANT_WIDTHS = [272, 528, 2064, 16368]   # a partly filled wave in the last pass of each


# ------------------------------------------------------------------------- the model of the kernels
def _reduce(part, D, op="sum", wave_rows=False, mutant=None, c0=0):
    """part [M, D / 8] fp32 (one value per chunk) reduced as the kernels do: per thread over its
    passes, per wave over 64 lanes, then over the waves. wave_rows: one wave per row, D / 512 passes."""
    M, nch = part.shape
    T = 64 if wave_rows else P.row_threads(D)
    passes = D // 512 if wave_rows else MAXCH
    assert nch <= T * passes
    zero = 0.0 if op == "sum" else float("-inf")
    grid = torch.full((M, passes * T), zero)
    grid[:, :nch] = part
    live = torch.zeros(passes * T, dtype=torch.bool)
    live[:nch] = True
    if mutant == "skip_chunk":
        grid[:, c0] = zero
    if mutant == "double_chunk":
        grid[:, c0] *= 2
    grid, live = grid.view(M, passes, T // 64, 64), live.view(passes, T // 64, 64)
    if mutant == "drop_last_pass":
        grid[:, MAXCH - 1:] = zero
    if mutant == "drop_partial_wave":
        n_live = live.sum(-1)
        grid[:, (n_live > 0) & (n_live < 64)] = zero
    if op == "sum":
        acc = torch.zeros(M, T // 64, 64)
        for i in range(passes):
            acc = acc + grid[:, i]
        waves = acc.sum(-1)
        tot = torch.zeros(M)
        for w in range(T // 64):
            tot = tot + waves[:, w]
        return tot
    return grid.amax((1, 2, 3)).clamp_min(0.0)


def _chunk_sum(v):
    """[M, D] -> [M, D / 8]: the eight elements of a chunk added in order."""
    c = v.view(v.shape[0], -1, 8)
    s = torch.zeros(c.shape[:2])
    for e in range(8):
        s = s + c[..., e]
    return s


def _take_neighbour_chunk(w, c0):
    w = w.clone()
    src = c0 + 1 if (c0 + 1) * 8 < w.numel() else c0 - 1
    w[c0 * 8:c0 * 8 + 8] = w[src * 8:src * 8 + 8]
    return w


def model_rmsnorm(x, w, eps, resid=None, wave_rows=False, mutant=None, c0=0):
    D = x.shape[1]
    v = x.to(BF16).float()
    new_resid = None
    if resid is not None:
        v = v + resid.to(BF16).float()
        new_resid = v.to(BF16)
    ss = _reduce(_chunk_sum(v * v), D, "sum", wave_rows, mutant, c0)
    inv = torch.rsqrt(ss / D + torch.tensor(eps, dtype=torch.float32))
    wv = w.to(BF16).float()
    if mutant == "w_neighbour_chunk":
        wv = _take_neighbour_chunk(wv, c0)
    return (v * inv[:, None] * wv).to(BF16), new_resid


def model_layernorm(x, g, b, eps, dtype=BF16, resid=None, mutant=None, c0=0, which="var"):
    D = x.shape[1]
    v = x.to(dtype).float()
    if resid is not None:
        v = v + resid.to(dtype).float()
    mean = _reduce(_chunk_sum(v), D, "sum", False, mutant if which == "mean" else None, c0) / D
    d = v - mean[:, None]
    var = _reduce(_chunk_sum(d * d), D, "sum", False, mutant if which == "var" else None, c0) / D
    inv = torch.rsqrt(var + torch.tensor(eps, dtype=torch.float32))
    gv, bv = g.to(dtype).float(), b.to(dtype).float()
    if mutant == "w_neighbour_chunk":
        gv = _take_neighbour_chunk(gv, c0)
    if mutant == "b_neighbour_chunk":
        bv = _take_neighbour_chunk(bv, c0)
    return d * inv[:, None] * gv + bv      # fp32: the caller rounds (or quantises) it


def model_bert_rows(e, dtype=BF16, types="given", mutant=None):
    """The kernel's fp32 sum word[ids] + pos[positions] + type[types or 0]."""
    word = e.word if types == "given" else e.word_none
    ty = e.types.long() if (types == "given" and mutant != "types_ignored") else torch.zeros_like(e.types).long()
    rows = word[e.ids.long()].to(dtype).float() + e.pos[e.positions.long()].to(dtype).float()
    return rows + e.type[ty].to(dtype).float()


def model_quant(v, D, mutant=None, c0=0, wave_rows=False):
    """quant_fp8's rule on fp32 rows v: (codes e4m3, scale fp32)."""
    amax = _reduce(v.abs().view(v.shape[0], -1, 8).amax(-1), D, "max", wave_rows, mutant, c0)
    sc = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    inv = 1.0 / sc
    return (v * inv[:, None]).clamp(-448, 448).to(FP8), sc


def model_pool(case, mode, dtype=BF16, mutant=None, at=None):
    """(out32, out16) of pool_l2norm; mutant drop_token / double_token at = (sequence, token)."""
    h = case.h.to(dtype).float()
    cu = case.cu.long()
    lens = cu[1:] - cu[:-1]
    v = h[cu[:-1]]
    if mode == 1:
        wgt = torch.ones(h.shape[0])
        if mutant in ("drop_token", "double_token"):
            wgt[int(cu[at[0]]) + at[1]] = 0.0 if mutant == "drop_token" else 2.0
        seg = torch.repeat_interleave(torch.arange(case.B), lens)
        sums = torch.zeros(case.B, case.D).index_add_(0, seg, h * wgt[:, None])
        invn = 1.0 / lens.clamp_min(1).float()
        v = torch.where((lens > 0)[:, None], sums * invn[:, None], v)
    chunk_mutant = mutant if mutant in ("skip_chunk", "double_chunk") else None
    ss = _reduce(_chunk_sum(v * v), case.D, "sum", False, chunk_mutant, at[0] if chunk_mutant else 0)
    inv = torch.where(ss > 0, torch.rsqrt(ss), torch.ones_like(ss))
    out = v * inv[:, None]
    return out, out.to(BF16)


def model_rope(case, rotate_q=True, mutant=None):
    """fp32 rope_cache on the case's qkv -> (qkv, k rows, v rows), all bf16-rounded."""
    H, Hkv, D, T = case.H, case.Hkv, case.D, case.T
    pos = case.pos.long()
    if mutant == "pos_plus_1":
        pos = pos + 1
    if mutant == "pos_minus_1":
        pos = pos - 1
    cs = P.rope_table_90(case.max_seq + 1, D)[pos]       # [T, D/2, 2]
    c, s = cs[:, None, :, 0], cs[:, None, :, 1]
    if mutant == "swap_cos_sin":
        c, s = s, c
    if mutant == "negate_sin":
        s = -s
    if mutant == "next_pair_angle":
        c, s = c.roll(-1, dims=2), s.roll(-1, dims=2)
    x = case.qkv.to(BF16).float().view(T, H + 2 * Hkv, D).clone()
    lo = 0 if rotate_q else H
    x1, x2 = x[:, lo:H + Hkv, 0::2], x[:, lo:H + Hkv, 1::2]
    x[:, lo:H + Hkv] = torch.stack([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).flatten(-2)
    x = x.to(BF16)
    return x.reshape(T, -1), x[:, H:H + Hkv], x[:, H + Hkv:]


# ------------------------------------------------------------------- the model passes, references hold
@pytest.mark.parametrize("D", GPU_WIDTHS)
def test_model_passes_and_references_hold(D):
    c = P.rms_case(D)
    c.check_reference()
    for wave_rows in ((False, True) if D in P.ROWS_WIDTHS else (False,)):
        y, _ = model_rmsnorm(c.h, c.w, c.eps, wave_rows=wave_rows)
        P.check_rms(y, c, f"rmsnorm D={D}")
        y, r = model_rmsnorm(c.x_resid, c.w, c.eps, resid=c.resid, wave_rows=wave_rows)
        P.check_rms(y, c, f"rmsnorm + resid D={D}")
        assert torch.equal(r.double(), c.h)
        codes, sc = model_quant(y.float(), D, wave_rows=wave_rows)
        bad_s, bad_c = P.quant_rule_failures(codes, sc, y)
        assert not bool(bad_s.any()) and not bool(bad_c.any())
    ln = P.ln_case(D)
    ln.check_reference()
    e = P.EmbedLnCase(ln)
    e.check_reference()
    for dtype in (BF16, F16) if D in P.F16_WIDTHS else (BF16,):
        P.check_ln(model_layernorm(ln.h, ln.g, ln.b, ln.eps, dtype).to(dtype), ln.t, ln.b, f"layernorm {dtype} D={D}")
        P.check_ln(model_layernorm(ln.x_resid, ln.g, ln.b, ln.eps, dtype, resid=ln.resid).to(dtype), ln.t, ln.b)
        for types in ("given", "none"):
            rows = model_bert_rows(e, dtype, types)
            assert torch.equal(rows.double(), ln.h)
    yf = model_layernorm(ln.h, ln.g, ln.b, ln.eps)
    bad_s, bad_c = P.fused_fp8_failures(*model_quant(yf, D), ln.t, ln.b)
    assert not bool(bad_s.any()) and not bool(bad_c.any())
    q = P.QuantCase(D)
    q.check_reference()
    codes, sc = model_quant(q.x.to(BF16).float(), D)
    assert torch.equal(codes.view(torch.uint8), q.codes) and torch.equal(sc, q.scale)
    pc = P.PoolCase(D)
    pc.check_reference()
    for mode in (0, 1):
        for dtype in (BF16, F16) if D in P.F16_WIDTHS and mode == 1 else (BF16,):
            o32, o16 = model_pool(pc, mode, dtype)
            assert not bool(P.pool_failures32(o32, pc.ref(mode)).any())
            assert not bool(P.failures(o16, pc.ref(mode)).any())


@pytest.mark.parametrize("H,Hkv,D", P.ROPE_SHAPES)
def test_rope_model_passes_and_reference_holds(H, Hkv, D):
    from docagents_amd.ops import reference as R
    c = P.RopeCase(H, Hkv, D)
    items = c.check_reference()
    assert (items > 256) == ((H, Hkv, D) in P.ROPE_SHAPES[:2])
    for rq in (True, False):
        got = model_rope(c, rq)
        for g, want in zip(got, c.exact(rq)):
            assert torch.equal(g.double(), want)
        for rows in c.exact(rq)[1:]:                      # the fp8 cache holds the rows exactly
            codes, s = R.quant_weight_fp8_pow2(rows.reshape(-1, D).to(BF16))
            assert torch.equal(codes.double() * s.double()[:, None], rows.reshape(-1, D))
    kc, vc = c.caches()
    untouched = torch.ones(kc.shape[:3], dtype=torch.bool)
    untouched[c.slot.long()[:, None], torch.arange(Hkv)[None, :], c.pos.long()[:, None]] = False
    assert bool((kc[untouched] == P.CACHE_FILL).all()) and int((~untouched).sum()) == c.T * Hkv


def test_embed_inputs():
    for D in P.EMBED_WIDTHS:
        assert P.exact_in(P.embed_table(D), BF16)
    ids = P.embed_ids().tolist()
    assert 0 in ids and 22 in ids and len(set(ids)) < len(ids) == 37


# ------------------------------------------------------------------------------------- the mutants
def _c0s(D):
    """The chunks a mutant is placed at: the first, one in the middle, the last (at the widest case
    the last alone: it lives in the eighth pass and in the partly filled wave)."""
    n = D // 8
    return sorted({0, n // 2 + 1, n - 1}) if D < 8192 else [n - 1]


SUM_MUTANTS = ("skip_chunk", "double_chunk", "drop_partial_wave", "w_neighbour_chunk")
# (mutant, D): every mutant at every width; the dropped last pass where there is an eighth pass
SUM_CASES = [(m, D) for D in MUTANT_WIDTHS for m in SUM_MUTANTS] + [("drop_last_pass", 16368)]


@pytest.mark.parametrize("mutant,D", SUM_CASES)
def test_rmsnorm_mutant_fails(mutant, D):
    """One chunk skipped in the sum of squares, one counted twice, the last MAXCH pass dropped (it
    exists at D > 7 * 2048 only), the lanes of a partly filled wave dropped, w taken from the
    neighbouring chunk: each fails the RMSNorm criterion, with and without the residual, and through
    rmsnorm_q8's rule."""
    c = P.rms_case(D)
    for c0 in _c0s(D):
        y, _ = model_rmsnorm(c.h, c.w, c.eps, mutant=mutant, c0=c0)
        assert int(P.failures(y, c.ref).sum()) > 0, f"{mutant} at chunk {c0} passes"
        y, _ = model_rmsnorm(c.x_resid, c.w, c.eps, resid=c.resid, mutant=mutant, c0=c0)
        assert int(P.failures(y, c.ref).sum()) > 0, f"{mutant} at chunk {c0} passes with resid"


@pytest.mark.parametrize("D", P.ROWS_WIDTHS)
@pytest.mark.parametrize("mutant", ("skip_chunk", "double_chunk", "w_neighbour_chunk"))
def test_rmsnorm_rows_mutant_fails(mutant, D):
    c = P.rms_case(D)
    for c0 in _c0s(D):
        y, _ = model_rmsnorm(c.h, c.w, c.eps, wave_rows=True, mutant=mutant, c0=c0)
        assert int(P.failures(y, c.ref).sum()) > 0


@pytest.mark.parametrize("which", ("mean", "var"))
@pytest.mark.parametrize("mutant,D", SUM_CASES + [("b_neighbour_chunk", D) for D in MUTANT_WIDTHS])
def test_layernorm_mutant_fails(mutant, D, which):
    """The same mutants in the mean sum and in the variance sum, and g / b from the neighbouring
    chunk, under the LayerNorm bound in bf16 (the wider of the two)."""
    ln = P.ln_case(D)
    for c0 in _c0s(D):
        y = model_layernorm(ln.h, ln.g, ln.b, ln.eps, BF16, mutant=mutant, c0=c0, which=which).to(BF16)
        assert int(P.ln_failures(y, ln.t, ln.b).sum()) > 0, f"{mutant} in {which} at chunk {c0} passes"


@pytest.mark.parametrize("D", [16, 272, 3072])
def test_types_ignored_fails(D):
    ln = P.ln_case(D)
    e = P.EmbedLnCase(ln)
    rows = model_bert_rows(e, BF16, "given", mutant="types_ignored")
    y = model_layernorm(rows, ln.g, ln.b, ln.eps).to(BF16)
    bad = P.ln_failures(y, ln.t, ln.b).any(1)
    assert bool(bad[e.types.bool()].all())          # every row whose type is 1


@pytest.mark.parametrize("D", MUTANT_WIDTHS)
def test_missed_maximum_fails(D):
    """The row maximum missed in one chunk: the row whose +-448 lives there gets another scale and
    saturated codes; through the fused fp8 output and rmsnorm_q8's rule too."""
    q = P.QuantCase(D)
    ln, c = P.ln_case(D), P.rms_case(D)
    for c0 in _c0s(D):
        codes, sc = model_quant(q.x.float(), D, "skip_chunk", c0)
        assert sc[c0] != q.scale[c0] and not torch.equal(codes.view(torch.uint8)[c0], q.codes[c0])
        keep = torch.arange(D // 8) != c0
        assert torch.equal(sc[keep], q.scale[keep])
        yf = model_layernorm(ln.h, ln.g, ln.b, ln.eps)
        bad_s, bad_c = P.fused_fp8_failures(*model_quant(yf, D, "skip_chunk", c0), ln.t, ln.b)
        assert bool(bad_s[c0])    # the codes follow the kernel's own scale: the scale shows it
        y, _ = model_rmsnorm(c.h, c.w, c.eps)
        bad_s, bad_c = P.quant_rule_failures(*model_quant(y.float(), D, "skip_chunk", c0), y)
        assert bool(bad_s[c0]) and bool(bad_c[c0].any())


@pytest.mark.parametrize("mutant", ("drop_token", "double_token"))
def test_pool_token_mutant_fails(mutant):
    """One token dropped from / counted twice in a mean, at every probe sequence longer than one token
    and every token of it that matters (t*, a neighbour, the first, the last)."""
    pc = P.PoolCase(272)
    ref = pc.ref(1)
    cu = pc.cu.tolist()
    for b in range(15 + 2):
        L = cu[b + 1] - cu[b]
        if pc.kinds[b] != "probe" or (L == 1 and mutant == "drop_token"):
            continue
        for t in sorted({0, L // 2, L - 1, min(1, L - 1)}):
            o32, o16 = model_pool(pc, 1, mutant=mutant, at=(b, t))
            assert bool(P.pool_failures32(o32, ref)[b].any()) or L == 1, (mutant, L, t)
    o32, _ = model_pool(pc, 1, mutant="skip_chunk", at=(33, 0))
    assert int(P.pool_failures32(o32, ref).any(1).sum()) >= 1


def test_pool_doubling_the_only_token_is_invisible():
    """L = 1: a mean over the one token counted twice is 2 v, and normalising removes the factor. No
    input can show it; the sequences of length 2 and more do."""
    pc = P.PoolCase(16)
    b = pc.kinds.index("probe")
    assert pc.cu.tolist()[b + 1] - pc.cu.tolist()[b] == 1
    o32, _ = model_pool(pc, 1, mutant="double_token", at=(b, 0))
    assert not bool(P.pool_failures32(o32, pc.ref(1)).any())


ROPE_MUTANTS = ("swap_cos_sin", "negate_sin", "next_pair_angle", "pos_plus_1", "pos_minus_1")


@pytest.mark.parametrize("mutant", ROPE_MUTANTS)
@pytest.mark.parametrize("H,Hkv,D", P.ROPE_SHAPES[2:])
def test_rope_mutant_fails(mutant, H, Hkv, D):
    """cos and sin swapped, sin negated, pair i + 1's angle, position p +- 1: every token's q and k
    rows differ from the exact rotation (a negated sin: every token at an odd position; at p = 2 mod 4
    every angle of the 90-degree table is a multiple of 180 degrees and its sine is 0)."""
    c = P.RopeCase(H, Hkv, D)
    got, k, _ = model_rope(c, True, mutant)
    want, wk, _ = c.exact(True)
    tokens = c.pos % 2 == 1 if mutant == "negate_sin" else torch.ones(c.T, dtype=torch.bool)
    assert int(tokens.sum()) >= c.T // 2
    assert bool((got.double() != want).any(1)[tokens].all()) and bool((k.double() != wk).flatten(1).any(1)[tokens].all())


# ------------------------------------------------------------------------------- negative control
def _old_close(got, ref, atol, rtol=0.02):
    got, ref = got.float(), ref.float()
    return int(((got - ref).abs() > atol + rtol * ref.abs()).sum())


def test_old_criteria_on_gaussian_inputs():
    """Negative control: the inputs and criteria of test_kernels_gpu.py (Gaussian rows; test_rmsnorm
    at D = 3072, test_layernorm_and_embed at 384 and 1024, test_pool_l2norm, test_rope_cache at
    (8, 2, 128), test_gemm_fp8_matches_dequantized_reference's quant_fp8 check at 300 x 768) under
    the mutants above, as outputs flagged by the old criterion / outputs the mutant moved. The inputs
    are seeded, so the outcome is asserted:
      rmsnorm 37 x 3072       skip_chunk 0 / 25703   double_chunk 0 / 25122   w_neighbour_chunk 281 / 296
      layernorm 19 x 1024     skip_chunk (var) 0 / 8245   double_chunk (var) 0 / 8187
                              skip_chunk (mean) 0 / 7543   b_neighbour_chunk 133 / 151
      layernorm 19 x 384      drop_partial_wave 7296 / 7296 (its one wave is the partly filled one)
      pool mean 4 x 768       drop_token 534 / 768   double_token 518 / 768   (of the 30-token sequence)
      rope 21 x (8, 2, 128)   swap_cos_sin 25809 / 26765   negate_sin 18428 / 23746
                              next_pair_angle 11576 / 20572   pos_plus_1 8311 / 17999
      quant_fp8 300 x 768     missed maximum: 4 of 300 rows flagged (those whose maximum is in the chunk)
      bert_embed_ln           types ignored: not reachable, types is None in every call
    PASS the old criteria unnoticed: a chunk skipped or doubled in any sum of RMSNorm or LayerNorm
    (inv moves by 8 / (2 D), far below rtol). The others do NOT pass, so they are not forced: a whole
    chunk of Gaussian weights, a wrong angle or a token missing from a 30-token Gaussian mean moves
    many outputs far, and the old criterion flags those among them that exceed its tolerance; the
    small-angle pairs (the upper part of every head at pos <= 60) stay unflagged, which is why up to
    half of the moved RoPE outputs are, and a missed maximum shows only in the 1 % of rows whose
    maximum lies in that chunk. On the probe inputs every row a mutant touches fails (the tests
    above). The dropped last pass needs D > 14336, which no old test launches."""
    from docagents_amd.ops import reference as R
    g = torch.Generator().manual_seed(1)

    def rand(*shape):
        return torch.randn(*shape, generator=g).to(BF16)

    seen = {}
    x, w = rand(37, 3072), rand(3072)
    ref = R.rmsnorm(x, w, 1e-5)
    base, _ = model_rmsnorm(x, w, 1e-5)
    assert _old_close(base, ref, 0.02) == 0
    for m in ("skip_chunk", "double_chunk", "w_neighbour_chunk"):
        y, _ = model_rmsnorm(x, w, 1e-5, mutant=m, c0=193)
        seen["rms " + m] = (_old_close(y, ref, 0.02), int((y != base).sum()))
    for D, muts in ((1024, (("skip_chunk", "var"), ("double_chunk", "var"), ("skip_chunk", "mean"),
                            ("b_neighbour_chunk", "var"))), (384, (("drop_partial_wave", "var"),))):
        x, gg, b = rand(19, D), rand(D), rand(D)
        ref = R.layernorm(x, gg, b, 1e-12)
        base = model_layernorm(x, gg, b, 1e-12).to(BF16)
        assert _old_close(base, ref, 0.03) == 0
        for m, which in muts:
            y = model_layernorm(x, gg, b, 1e-12, mutant=m, c0=D // 16 + 1, which=which).to(BF16)
            seen[f"ln{D} {m} {which}"] = (_old_close(y, ref, 0.03), int((y != base).sum()))

    class Pool:
        D, B = 768, 4
        h = rand(50, 768).float()
        cu = torch.tensor([0, 5, 5, 20, 50], dtype=torch.int32)
    ref = R.pool_l2norm(Pool.h.to(BF16), Pool.cu, 1)
    base, _ = model_pool(Pool, 1)
    assert _old_close(base, ref, 2e-3) == 0
    for m in ("drop_token", "double_token"):
        y, _ = model_pool(Pool, 1, mutant=m, at=(3, 11))
        seen["pool " + m] = (_old_close(y, ref, 2e-3), int((y != base).sum()))

    H, Hkv, D, T = 8, 2, 128, 21
    qkv = rand(T, (H + 2 * Hkv) * D)
    pos = torch.arange(T) * 3
    table = R.rope_table(129, D, 10000.0)

    def rope(mutant=None):
        p = pos + 1 if mutant == "pos_plus_1" else pos
        cs = table[p]
        c, s = cs[:, None, :, 0], cs[:, None, :, 1]
        if mutant == "swap_cos_sin":
            c, s = s, c
        if mutant == "negate_sin":
            s = -s
        if mutant == "next_pair_angle":
            c, s = c.roll(-1, dims=2), s.roll(-1, dims=2)
        x = qkv.float().view(T, H + 2 * Hkv, D).clone()
        x1, x2 = x[:, :H + Hkv, 0::2], x[:, :H + Hkv, 1::2]
        x[:, :H + Hkv] = torch.stack([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).flatten(-2)
        return x.to(BF16).reshape(T, -1)
    ref = R.rope_cache(qkv.clone(), pos.int(), table, H, Hkv, D)
    base = rope()
    assert _old_close(base, ref, 0.02) == 0
    for m in ("swap_cos_sin", "negate_sin", "next_pair_angle", "pos_plus_1"):
        y = rope(m)
        seen["rope " + m] = (_old_close(y, ref, 0.02), int((y != base).sum()))

    x = rand(300, 768)
    rq, rs = R.quant_fp8(x)
    _, sc = model_quant(x.float(), 768, "skip_chunk", 40)
    seen["quant missed max"] = (int((~torch.isclose(sc, rs, rtol=1e-6)).sum()), 300)

    print(f"old criteria: (flagged, moved) = {seen}")
    for name, (flagged, moved) in seen.items():
        assert 0 < moved and flagged <= moved, (name, flagged, moved)
    passes = {n for n, (flagged, _) in seen.items() if flagged == 0}
    assert passes == {"rms skip_chunk", "rms double_chunk", "ln1024 skip_chunk var", "ln1024 double_chunk var",
                      "ln1024 skip_chunk mean"}, passes
