"""The row kernels of ops/csrc/norm.hip, rope_cache_kernel and rope_cache_kv8 on the inputs of
tests/row_probes.py: spike rows (every chunk carries some row's whole sum), dense rows with separated
weights, exact RoPE rotations. A dropped or doubled chunk, a weight from the neighbouring chunk, a
wrong angle or a missed maximum fails; tests/test_row_probes_cpu.py shows that on a model of the
kernels. Every tolerance is bit for bit / either neighbour or derived in row_probes.py.

One launch per case: M = D / 8 spike rows + 3 dense rows (+ 3 constant rows for LayerNorm)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from docagents_amd.ops import kernels as K  # noqa: E402
from docagents_amd.ops import reference as R  # noqa: E402

import row_probes as P  # noqa: E402
from row_probes import BF16, F16, FP8  # noqa: E402

DEV = "cuda"
WIDTHS_8 = (8,) + P.WIDTHS
FILL = 5.0


def _dev(t, dtype=BF16):
    return t.to(dtype).to(DEV)


def _none_bad(mask, what):
    n = int(mask.sum())
    assert n == 0, f"{what}: {n} / {mask.numel()} miss; first at {tuple(int(i) for i in mask.nonzero()[0])}"


# ------------------------------------------------------------------------------------------ RMSNorm
def _rms_all(D, route_m):
    c = P.rms_case(D)
    w = _dev(c.w)
    what = f"rmsnorm D={D} route_m={route_m}"
    y = K.rmsnorm(_dev(c.h), w, c.eps, route_m=route_m)
    P.check_rms(y, c, what)
    resid = _dev(c.resid.double())
    y2 = K.rmsnorm(_dev(c.x_resid), w, c.eps, resid=resid, route_m=route_m)
    P.check_rms(y2, c, what + " resid")
    assert torch.equal(resid.double().cpu(), c.h), what + ": the updated residual stream is not x + resid"
    assert torch.equal(y2, y)
    # row-padded input and output, the poison in the gap
    out = P.padded(torch.full((c.M, D), FILL, dtype=BF16, device=DEV))
    K.rmsnorm(P.padded(_dev(c.h)), w, c.eps, out=out, route_m=route_m)
    assert torch.equal(out, y), what + " padded"
    gap = torch.as_strided(out, (c.M, 16), (out.stride(0), 1), out.storage_offset() + D)
    assert bool((gap == P.POISON).all()), what + ": the padding of out was written"
    if D % 16:
        return  # the e4m3 wrappers take rows of whole 16-byte groups only
    # straight to e4m3: the rule on the bf16 row just checked; spike rows: +-448 at the spike
    codes, scale = K.rmsnorm_q8(_dev(c.h), w, c.eps, route_m=route_m)
    bad_s, bad_c = P.quant_rule_failures(codes, scale, y)
    _none_bad(bad_s, what + " q8 scale")
    _none_bad(bad_c, what + " q8 codes")
    n = D // 8
    cv = codes[:n].float().cpu()
    want = torch.zeros(n, D)
    want[torch.arange(n), P.spike_cols(n)] = 448.0 * torch.sign(P.spike_values(n)).float()
    assert torch.equal(cv, want), what + ": q8 spike rows"
    rep = ~P.G.rounded_mask(c.ref).any(1)          # rows bf16 holds exactly: R.quant_fp8 of the exact row
    rq, rs = R.quant_fp8(c.ref[rep].to(BF16))
    assert torch.equal(scale.cpu()[rep], rs) and torch.equal(codes.cpu()[rep].view(torch.uint8), rq.view(torch.uint8))
    codes_p = torch.full((c.M, D + (16 if D % 16 == 0 else 24)), 0x55, dtype=torch.uint8, device=DEV).view(FP8)
    K.rmsnorm_q8(P.padded(_dev(c.h)), w, c.eps, out=codes_p[:, :D], route_m=route_m)
    assert torch.equal(codes_p[:, :D].view(torch.uint8), codes.view(torch.uint8))
    assert bool((codes_p[:, D:].view(torch.uint8) == 0x55).all())


@pytest.mark.parametrize("D", WIDTHS_8)
def test_rmsnorm_one_workgroup_per_row(D):
    _rms_all(D, 0)


@pytest.mark.parametrize("D", P.ROWS_WIDTHS)
def test_rmsnorm_one_wave_per_row(D):
    """route_m = 1024 selects rmsnorm_rows_kernel / rmsnorm_q8_rows_kernel; M = D / 8 + 3 leaves the
    last workgroup partly empty."""
    assert (D // 8 + P.N_DENSE) % 4 != 0
    _rms_all(D, 1024)


# ---------------------------------------------------------------------------------------- LayerNorm
def _ln_forms(D, dtype):
    ln = P.ln_case(D)
    g, b = _dev(ln.g, dtype), _dev(ln.b, dtype)
    layernorm = K.layernorm if dtype == BF16 else K.layernorm_f16
    embed_ln = K.bert_embed_ln if dtype == BF16 else K.bert_embed_ln_f16
    what = f"layernorm {dtype} D={D}"
    P.check_ln(layernorm(_dev(ln.h, dtype), g, b, ln.eps), ln.t, ln.b, what)
    P.check_ln(layernorm(_dev(ln.x_resid, dtype), g, b, ln.eps, resid=_dev(ln.resid.double(), dtype)), ln.t, ln.b,
               what + " resid")
    e = P.EmbedLnCase(ln)
    ids, ps, ty = e.ids.to(DEV), e.positions.to(DEV), e.types.to(DEV)
    pos, typ = _dev(e.pos, dtype), _dev(e.type, dtype)
    P.check_ln(embed_ln(ids, ps, ty, _dev(e.word, dtype), pos, typ, g, b, ln.eps), ln.t, ln.b, what + " embed, types")
    P.check_ln(embed_ln(ids, ps, None, _dev(e.word_none, dtype), pos, typ, g, b, ln.eps), ln.t, ln.b,
               what + " embed, types=None")
    return ln, e


@pytest.mark.parametrize("D", WIDTHS_8)
def test_layernorm_and_bert_embed_ln(D):
    ln, e = _ln_forms(D, BF16)
    # fused fp8 output: the spike rows (and the others) against the fp64 row
    g, b = _dev(ln.g), _dev(ln.b)
    y, yq, ys = K.layernorm(_dev(ln.h), g, b, ln.eps, fp8_out=True)
    P.check_ln(y, ln.t, ln.b, f"layernorm fp8_out D={D}")
    bad_s, bad_c = P.fused_fp8_failures(yq, ys, ln.t, ln.b)
    _none_bad(bad_s, f"layernorm fp8_out D={D} scale")
    _none_bad(bad_c, f"layernorm fp8_out D={D} codes")
    y, yq, ys = K.bert_embed_ln(e.ids.to(DEV), e.positions.to(DEV), e.types.to(DEV), _dev(e.word), _dev(e.pos),
                                _dev(e.type), g, b, ln.eps, fp8_out=True)
    P.check_ln(y, ln.t, ln.b, f"bert_embed_ln fp8_out D={D}")
    bad_s, bad_c = P.fused_fp8_failures(yq, ys, ln.t, ln.b)
    _none_bad(bad_s, f"bert_embed_ln fp8_out D={D} scale")
    _none_bad(bad_c, f"bert_embed_ln fp8_out D={D} codes")


@pytest.mark.parametrize("D", P.F16_WIDTHS)
def test_layernorm_and_bert_embed_ln_f16(D):
    _ln_forms(D, F16)


# -------------------------------------------------------------------------------------------- pool
@pytest.mark.parametrize("D", WIDTHS_8)
def test_pool_l2norm(D):
    pc = P.PoolCase(D)
    h, cu = _dev(pc.h), pc.cu.to(DEV)
    for mode in (0, 1):
        ref = pc.ref(mode, DEV)
        o32 = torch.full((pc.B, D), FILL, device=DEV)
        o16 = torch.full((pc.B, D), FILL, device=DEV, dtype=BF16)
        K.pool_l2norm(h, cu, mode, out32=o32, out16=o16)
        _none_bad(P.pool_failures32(o32, ref), f"pool_l2norm mode {mode} D={D} fp32")
        _none_bad(P.failures(o16, ref), f"pool_l2norm mode {mode} D={D} bf16")
        assert torch.equal(K.pool_l2norm(h, cu, mode), o32) and torch.equal(K.pool_l2norm(h, cu, mode, out16=o16), o16)


@pytest.mark.parametrize("D", P.F16_WIDTHS)
def test_pool_l2norm_f16(D):
    pc = P.PoolCase(D)
    h, cu = _dev(pc.h, F16), pc.cu.to(DEV)
    for mode in (0, 1):
        ref = pc.ref(mode, DEV)
        o32 = torch.full((pc.B, D), FILL, device=DEV)
        o16 = torch.full((pc.B, D), FILL, device=DEV, dtype=BF16)
        K.pool_l2norm_f16(h, cu, mode, out32=o32, out16=o16)
        _none_bad(P.pool_failures32(o32, ref), f"pool_l2norm_f16 mode {mode} D={D} fp32")
        _none_bad(P.failures(o16, ref), f"pool_l2norm_f16 mode {mode} D={D} bf16")


# ------------------------------------------------------------------------------------------- quant
@pytest.mark.parametrize("D", P.WIDTHS)
def test_quant_fp8_rows(D):
    q = P.QuantCase(D)
    codes, scale = K.quant_fp8(_dev(q.x))
    assert torch.equal(scale.cpu(), q.scale), f"quant_fp8 D={D}: scales"
    assert torch.equal(codes.cpu().view(torch.uint8), q.codes), f"quant_fp8 D={D}: codes"


# ------------------------------------------------------------------------------------------- embed
@pytest.mark.parametrize("D", P.EMBED_WIDTHS)
def test_embed(D):
    table, ids = _dev(P.embed_table(D)), P.embed_ids().to(DEV)
    assert torch.equal(K.embed(ids, table), table[ids.long()])


# -------------------------------------------------------------------------------------------- RoPE
@functools.lru_cache(maxsize=4)
def _rope(H, Hkv, D):
    c = P.RopeCase(H, Hkv, D)
    c.check_reference()
    return c


@pytest.mark.parametrize("rotate_q", [True, False])
@pytest.mark.parametrize("H,Hkv,D", P.ROPE_SHAPES)
def test_rope_cache(H, Hkv, D, rotate_q):
    c = _rope(H, Hkv, D)
    pos, slot, cs = c.pos.to(DEV), c.slot.to(DEV), c.cs.to(DEV)
    want, _, _ = c.exact(rotate_q)
    kc_want, vc_want = c.caches(rotate_q)
    qkv = _dev(c.qkv)
    kc = torch.full(kc_want.shape, P.CACHE_FILL, dtype=BF16, device=DEV)
    vc = kc.clone()
    K.rope_cache(qkv, pos, cs, H, Hkv, D, slot=slot, k_cache=kc, v_cache=vc, rotate_q=rotate_q)
    assert torch.equal(qkv.double().cpu(), want)
    assert torch.equal(kc.double().cpu(), kc_want) and torch.equal(vc.double().cpu(), vc_want)
    qkv = _dev(c.qkv)
    K.rope_cache(qkv, pos, cs, H, Hkv, D, rotate_q=rotate_q)      # no caches
    assert torch.equal(qkv.double().cpu(), want)


@pytest.mark.parametrize("rotate_q", [True, False])
@pytest.mark.parametrize("H,Hkv,D", P.ROPE_SHAPES)
def test_rope_cache_kv8(H, Hkv, D, rotate_q):
    """Codes and scales are quant_weight_fp8_pow2 of the EXACT rotated rows (the reference's, not the
    kernel's own output); rows that are not addressed keep the fill."""
    c = _rope(H, Hkv, D)
    pos, slot, cs = c.pos.to(DEV), c.slot.to(DEV), c.cs.to(DEV)
    want, k, v = c.exact(rotate_q)
    shape = (P.ROPE_SLOTS, Hkv, c.max_seq, D)
    kq = torch.full(shape, 0x55, dtype=torch.uint8, device=DEV)
    vq = kq.clone()
    ks = torch.full(shape[:3], P.CACHE_FILL, device=DEV)
    vs = ks.clone()
    qkv = _dev(c.qkv)
    K.rope_cache_kv8(qkv, pos, cs, H, Hkv, D, slot, kq.view(FP8), vq.view(FP8), ks, vs, rotate_q=rotate_q)
    assert torch.equal(qkv.double().cpu(), want)
    sl, ps = c.slot.long(), c.pos.long()
    for rows, codes, scale in ((k, kq, ks), (v, vq, vs)):
        q, s = R.quant_weight_fp8_pow2(rows.reshape(-1, D).to(BF16))
        assert torch.equal(q.double() * s.double()[:, None], rows.reshape(-1, D))
        cw = torch.full(shape, 0x55, dtype=torch.uint8)
        sw = torch.full(shape[:3], P.CACHE_FILL)
        cw[sl, :, ps] = q.view(torch.uint8).view(c.T, Hkv, D)
        sw[sl, :, ps] = s.view(c.T, Hkv)
        assert torch.equal(codes.cpu(), cw) and torch.equal(scale.cpu(), sw)


# ------------------------------------------------------------------------------------- rejections
def _raises_and_writes_nothing(fn, *outs):
    before = [o.clone() for o in outs]
    with pytest.raises((ValueError, K.KernelError)):
        fn()
    torch.cuda.synchronize()
    for o, o0 in zip(outs, before):
        assert torch.equal(o.view(torch.uint8), o0.view(torch.uint8)), "a rejected call wrote"


@pytest.mark.parametrize("D", [16392, 20])
def test_bad_width_is_rejected(D):
    """D above 8 passes of 256 threads, or no multiple of 8: every wrapper raises and writes nothing."""
    M = 3
    x = torch.ones(M, D, dtype=BF16, device=DEV)
    x16 = x.to(F16)
    v, v16 = torch.ones(D, dtype=BF16, device=DEV), torch.ones(D, dtype=F16, device=DEV)
    out = torch.full((M, D), FILL, dtype=BF16, device=DEV)
    o16 = torch.full((M, D), FILL, dtype=F16, device=DEV)
    o32 = torch.full((M, D), FILL, device=DEV)
    oq = torch.full((M, D), 0x55, dtype=torch.uint8, device=DEV)
    sc = torch.full((M,), FILL, device=DEV)
    ids = torch.zeros(M, dtype=torch.int32, device=DEV)
    cu = torch.tensor([0, 1, 2, 3], dtype=torch.int32, device=DEV)
    _raises_and_writes_nothing(lambda: K.rmsnorm(x, v, 1e-5, out=out), out)
    _raises_and_writes_nothing(lambda: K.rmsnorm(x, v, 1e-5, resid=x.clone(), out=out), out)
    _raises_and_writes_nothing(lambda: K.rmsnorm_q8(x, v, 1e-5, out=oq.view(FP8), scale=sc), oq, sc)
    _raises_and_writes_nothing(lambda: K.quant_fp8(x, out=oq.view(FP8), scale=sc), oq, sc)
    _raises_and_writes_nothing(lambda: K.layernorm(x, v, v, 1e-12, out=out), out)
    _raises_and_writes_nothing(lambda: K.layernorm(x, v, v, 1e-12, resid=x, out=out), out)
    _raises_and_writes_nothing(lambda: K.layernorm(x, v, v, 1e-12, out=out, fp8_out=True), out)
    _raises_and_writes_nothing(lambda: K.layernorm_f16(x16, v16, v16, 1e-12, out=o16), o16)
    _raises_and_writes_nothing(lambda: K.bert_embed_ln(ids, ids, ids, x, x, x, v, v, 1e-12, out=out), out)
    _raises_and_writes_nothing(lambda: K.bert_embed_ln(ids, ids, None, x, x, x, v, v, 1e-12, out=out, fp8_out=True), out)
    _raises_and_writes_nothing(lambda: K.bert_embed_ln_f16(ids, ids, ids, x16, x16, x16, v16, v16, 1e-12, out=o16), o16)
    _raises_and_writes_nothing(lambda: K.embed(ids, x, out=out), out)
    for mode in (0, 1):
        _raises_and_writes_nothing(lambda: K.pool_l2norm(x, cu, mode, out32=o32, out16=out), o32, out)
        _raises_and_writes_nothing(lambda: K.pool_l2norm_f16(x16, cu, mode, out32=o32, out16=out), o32, out)


def test_rope_bad_head_dim_is_rejected():
    """A head dim that is no multiple of 8 (rope_cache_kv8: none but 64 / 96 / 128) raises; qkv and
    the caches stay as they were."""
    H, Hkv, T = 2, 1, 3
    pos = torch.tensor([1, 2, 3], dtype=torch.int32, device=DEV)
    slot = torch.zeros(T, dtype=torch.int32, device=DEV)
    for D in (20, 68):
        qkv = torch.full((T, (H + 2 * Hkv) * D), FILL, dtype=BF16, device=DEV)
        cs = P.rope_table_90(8, D, DEV)
        kc = torch.full((1, Hkv, 8, D), FILL, dtype=BF16, device=DEV)
        vc = kc.clone()
        _raises_and_writes_nothing(lambda: K.rope_cache(qkv, pos, cs, H, Hkv, D, slot=slot, k_cache=kc, v_cache=vc),
                                   qkv, kc, vc)
    for D in (68, 72, 16392):
        qkv = torch.full((T, (H + 2 * Hkv) * D), FILL, dtype=BF16, device=DEV)
        cs = P.rope_table_90(8, D, DEV)
        kq = torch.full((1, Hkv, 8, D), 0x55, dtype=torch.uint8, device=DEV)
        vq = kq.clone()
        ks = torch.full((1, Hkv, 8), FILL, device=DEV)
        vs = ks.clone()
        _raises_and_writes_nothing(lambda: K.rope_cache_kv8(qkv, pos, cs, H, Hkv, D, slot, kq.view(FP8), vq.view(FP8),
                                                            ks, vs), qkv, kq, vq, ks, vs)


def test_wrappers_refuse_operands_the_launcher_would_misread():
    """g / b / out32 / out16 of another dtype or stride: refused by the wrapper, nothing written."""
    D, M = 64, 3
    x = torch.ones(M, D, dtype=BF16, device=DEV)
    v = torch.ones(D, dtype=BF16, device=DEV)
    strided = torch.ones(2 * D, dtype=BF16, device=DEV)[::2]
    out = torch.full((M, D), FILL, dtype=BF16, device=DEV)
    cu = torch.tensor([0, 1, 2, 3], dtype=torch.int32, device=DEV)
    for g, b in ((v.float(), v), (v, v.float()), (strided, v), (v, strided), (v[:D - 8], v)):
        _raises_and_writes_nothing(lambda: K.layernorm(x, g, b, 1e-12, out=out), out)
        _raises_and_writes_nothing(lambda: K.bert_embed_ln(cu[:M], cu[:M], None, x, x, x, g, b, 1e-12, out=out), out)
    _raises_and_writes_nothing(lambda: K.layernorm(x, v, v, 1e-12, out=out.float()))
    bad32 = torch.full((M, D), FILL, dtype=BF16, device=DEV)
    _raises_and_writes_nothing(lambda: K.pool_l2norm(x, cu, 1, out32=bad32), bad32)
    bad16 = torch.full((M, D), FILL, device=DEV)
    _raises_and_writes_nothing(lambda: K.pool_l2norm(x, cu, 1, out16=bad16), bad16)
    wide = torch.full((M, 2 * D), FILL, device=DEV)
    _raises_and_writes_nothing(lambda: K.pool_l2norm(x, cu, 1, out32=wide[:, :D]), wide)
    _raises_and_writes_nothing(lambda: K.pool_l2norm_f16(x.to(F16), cu, 1, out32=wide[:, :D]), wide)
