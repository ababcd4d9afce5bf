"""Kernels write only their outputs: padded leading dimensions, ragged tiles and device-side state.

Every case runs the kernel twice: into a wrapper-allocated contiguous output, and into a view of a
pattern-filled frame (tests/kernel_frames.py) whose row stride is larger than N, with a framed
``resid`` of another stride where the op takes one. The two results must be bit-identical (the route
depends on M, N, K, never on strides, and these kernels are bit-reproducible between launches), every
element of the frame outside the view must still hold the pattern, and the contiguous result must
match the fp32 reference at the tolerance the kernel's own numerics test uses (so that two equally
wrong runs cannot pass). Kernels that write device-side state (KV caches, the sampler's bookkeeping)
are compared with the state's previous contents / the reference model of the bookkeeping.
"""
import numpy as np

import pytest
import torch

pytestmark = pytest.mark.gpu

from docagents_amd.ops import kernels as K  # noqa: E402
from docagents_amd.ops import reference as R  # noqa: E402

from kernel_frames import assert_frame_intact, fill_pattern, framed, guarded, holds_pattern  # noqa: E402

DEV = "cuda"
BF16 = torch.bfloat16
PADS = (8, 24)  # extra elements per row of a framed output (16-B multiples, two different strides)


def _rand(*shape, scale=1.0, dtype=BF16):
    return (torch.randn(*shape, device=DEV) * scale).to(dtype)


def _close(a, b, atol, rtol=0.02):
    a, b = a.float(), b.float()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = (err > tol).sum().item()
    assert bad == 0, f"{bad} / {a.numel()} mismatches, max err {err.max().item():.4g}"


def _frame(M, N, pad, dtype=BF16, **kw):
    return framed(M, N, dtype, pad, device=DEV, **kw)


def _framed_copy(t, pad):
    """``t`` [M, N] copied into the view of a fresh frame -> (buffer, view)."""
    buf, view = _frame(t.shape[0], t.shape[1], pad, dtype=t.dtype)
    view.copy_(t)
    return buf, view


def _write_check(run, M, nout, want, dtype=BF16, pads=PADS, resid=None):
    """run(out, resid) launches the kernel. For each pad: framed ``out`` (and ``resid`` framed with
    the other pad, then ``resid is out``) -> bit-identical to ``want`` (the contiguous launch), frames
    intact, the out-of-place residual unchanged."""
    for i, pad in enumerate(pads):
        buf, view = _frame(M, nout, pad, dtype)
        if resid is None:
            got = run(view, None)
            assert got.data_ptr() == view.data_ptr()
            assert torch.equal(view, want), f"framed out (pad {pad}) differs from the contiguous launch"
            assert_frame_intact(buf, view, f"out pad {pad}")
            continue
        rbuf, rview = _framed_copy(resid, pads[(i + 1) % len(pads)] + 32)  # never the stride of out
        assert rview.stride(0) != view.stride(0)
        run(view, rview)
        assert torch.equal(view, want), f"framed out / resid (pad {pad}) differs from the contiguous launch"
        assert_frame_intact(buf, view, f"out pad {pad}")
        assert_frame_intact(rbuf, rview, "resid frame")
        assert torch.equal(rview, resid), "out-of-place resid was modified"
        buf, view = _framed_copy(resid, pad)  # in place: resid is out
        run(view, view)
        assert torch.equal(view, want), f"in-place residual (pad {pad}) differs from the contiguous launch"
        assert_frame_intact(buf, view, f"in-place out pad {pad}")


# ------------------------------------------------------------------------------------- gemm routes
def _gemm_route_case(M, N, Kd, epi, atol, seed, pads=PADS, **route):
    torch.manual_seed(seed)
    a, w = _rand(M, Kd), _rand(N, Kd, scale=Kd ** -0.5)
    bias = _rand(N) if epi == K.EPI_BIAS else None
    resid = _rand(M, N) if epi == K.EPI_RESID else None
    nout = N // 2 if epi == K.EPI_SWIGLU else N

    def run(out, r):
        return K.gemm(a, w, bias=bias, epi=epi, resid=r, out=out, **route)
    want = run(None, resid)
    assert want.is_contiguous() and want.shape == (M, nout)
    _close(want, R.gemm(a, w, bias=bias, epi=epi, resid=resid), atol=atol)
    _write_check(run, M, nout, want, pads=pads, resid=resid)


EPIS = [K.EPI_NONE, K.EPI_BIAS, K.EPI_RESID, K.EPI_SWIGLU]


@pytest.mark.parametrize("M", [17, 77, 130])
@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("tile", [1, 2, 3, 9])
def test_gemm_tile_routes(tile, splits, M):
    """128x128, 64x128, 32x128 and 128x64 tiles, direct epilogue (splits 1) and split-K partials +
    gemm_splitk_reduce (splits 2): ragged M and N (392 = 3 x 128 + 8; SwiGLU 416 -> 208 outputs)."""
    for epi in EPIS:
        N = 416 if epi == K.EPI_SWIGLU else 392
        _gemm_route_case(M, N, 512, epi, 0.03, tile * 100 + splits * 10 + M + epi, tile=tile, splits=splits)


@pytest.mark.parametrize("N,Kd,epis", [(104, 512, (K.EPI_NONE, K.EPI_BIAS, K.EPI_RESID)), (96, 512, (K.EPI_SWIGLU,)),
                                       (8, 8192, (K.EPI_NONE, K.EPI_BIAS, K.EPI_RESID))])
def test_gemm_gemv_route(N, Kd, epis):
    """Tile 6 (M = 1): four rows per workgroup (N = 104: 26 waves, a ragged last workgroup), the
    SwiGLU form, and the two-waves-per-row long-row form (N = 8, K = 8192). The pad columns and the
    frame rows are the guard elements after the row."""
    for epi in epis:
        _gemm_route_case(1, N, Kd, epi, 0.03, N + epi, tile=6, splits=1)
        assert K.gemv_fusable(1, N, Kd, epi)


@pytest.mark.parametrize("Kd", [128, 192])
@pytest.mark.parametrize("tile", [7, 10])
def test_gemm8p_routes(tile, Kd):
    """Phase-split 256x256 / 128x256 tiles, one tile per workgroup: M = 300 and N = 264 leave a ragged
    last tile both ways (SwiGLU needs N % 32 == 0: 288 -> 144 outputs, still ragged)."""
    for epi in EPIS:
        N = 288 if epi == K.EPI_SWIGLU else 264
        _gemm_route_case(300, N, Kd, epi, 0.04, tile + Kd + epi, tile=tile, splits=1)


@pytest.mark.parametrize("tile", [7, 10])
def test_gemm8p_persistent_route(tile):
    """More tiles than CUs with the persistent tile loop on: 17 x 17 (tile 7) / 33 x 17 (tile 10) tiles,
    ragged M and N, residual epilogue out of place and in place."""
    prev = K.gemm8p_persist(1)
    try:
        _gemm_route_case(4100, 4104, 128, K.EPI_RESID, 0.04, tile, pads=(8,), tile=tile, splits=1)
    finally:
        K.gemm8p_persist(prev)


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_gemm4w_route(variant):
    """Four-wave 256x256 kernel (tile 13), its three schedules (K = 256: K / 64 even and >= 4)."""
    prev = K.gemm4w_variant(variant)
    try:
        for epi in EPIS:
            N = 288 if epi == K.EPI_SWIGLU else 264
            _gemm_route_case(300, N, 256, epi, 0.04, 13 + variant + epi, tile=13, splits=1)
    finally:
        K.gemm4w_variant(prev)


# ---------------------------------------------------------------------------------------- gemm_dk
@pytest.mark.parametrize("N", [48, 512, 1024, 12320])
@pytest.mark.parametrize("M", [3, 17, 33, 64])
def test_gemm_dk_writes(M, N):
    """gemm_dk: 16- / 32-row blocks, BN 16 (N = 48, 512, 1024), 32 (SwiGLU) and 64 (N = 12320); 33..64
    rows go to da_gemm_dk_splitk (64x128 tiles + reduce) unless an ssq_out forces the dk kernel's
    two-row-block form (N % 512 != 0). With ssq_out: nothing from element dk_parts(N, M) * 64 on."""
    Kd = 256
    for epi in (K.EPI_NONE, K.EPI_RESID, K.EPI_SWIGLU):
        if epi == K.EPI_SWIGLU and N % 32:
            continue  # N = 48: no whole gate / up groups
        torch.manual_seed(M * 7 + N + epi)
        a, w = _rand(M, Kd), _rand(N, Kd, scale=Kd ** -0.5)
        resid = _rand(M, N) if epi == K.EPI_RESID else None
        nout = N // 2 if epi == K.EPI_SWIGLU else N

        def run(out, r):
            return K.gemm_dk(a, w, epi=epi, resid=r, out=out)
        want = run(None, resid)
        _close(want, R.gemm(a, w, epi=epi, resid=resid), atol=0.03)
        _write_check(run, M, nout, want, resid=resid)
        if epi != K.EPI_RESID:
            continue
        parts = K.dk_parts(N, M)
        sbuf, ssq = guarded(parts * 64, torch.float32, guard=256, device=DEV)

        def run_ssq(out, r):
            return K.gemm_dk(a, w, epi=epi, resid=r, out=out, ssq_out=ssq)
        want2 = run_ssq(None, resid)
        if M <= K.DK_SPLITK_ABOVE:
            assert torch.equal(want2, want)  # same kernel with or without the sums
        else:  # 33..64 rows: the sums pick the reduce kernel (N % 512 == 0) or the dk kernel instead of split-K
            _close(want2, R.gemm(a, w, epi=epi, resid=resid), atol=0.03)
        _write_check(run_ssq, M, nout, want2, resid=resid)
        assert_frame_intact(sbuf, ssq, "ssq_out guards")
        sums = ssq.view(parts, 64)[:, :M].sum(0)
        _close(sums, want2.float().pow(2).sum(-1), atol=1e-2 * N, rtol=1e-3)


# -------------------------------------------------------------------------------- gemm_resid_norm
def test_gemm_resid_norm_rejects_uneven_split():
    """K = 448 is 7 k-tiles of 64: two splits do not divide them, and the launch must be refused
    before anything is written (so the two-split cases below run 7 k-tiles per split, K = 896)."""
    a, w, x, g = _rand(17, 448), _rand(392, 448), _rand(17, 392), _rand(392)
    obuf, oview = _frame(17, 392, 8)
    hbuf, hview = _frame(17, 392, 24)
    with pytest.raises(K.KernelError):
        K.gemm_resid_norm(a, w, x, g, 1e-5, out=oview, h_out=hview, splits=2)
    torch.cuda.synchronize()
    assert holds_pattern(obuf) and holds_pattern(hbuf)


@pytest.mark.parametrize("splits,Kd", [(1, 448), (2, 896)])
@pytest.mark.parametrize("M", [17, 64, 100])
def test_gemm_resid_norm_writes(M, splits, Kd):
    """Split-K GEMM + fused reduce / residual / RMSNorm: ``out`` (the new residual stream) and ``h_out``
    framed with different strides, resid out of place (a third stride) and in place (resid is out).
    7 k-tiles per split (not a multiple of the 4 in flight): K = 448 at one split, 896 at two."""
    torch.manual_seed(M + splits)
    N = 392
    a, w = _rand(M, Kd), _rand(N, Kd, scale=Kd ** -0.5)
    x, g = _rand(M, N), _rand(N) + 1.0
    out0 = torch.empty_like(x)
    h0 = K.gemm_resid_norm(a, w, x, g, 1e-5, out=out0, splits=splits)
    xr = x.clone()
    hr = R.gemm_resid_norm(a, w, xr, g, 1e-5, out=xr)
    _close(out0, xr, atol=0.03)
    _close(h0, hr, atol=0.05)
    for po, ph in ((8, 24), (24, 8)):
        obuf, oview = _frame(M, N, po)
        hbuf, hview = _frame(M, N, ph)
        rbuf, rview = _framed_copy(x, 40)
        K.gemm_resid_norm(a, w, rview, g, 1e-5, out=oview, h_out=hview, splits=splits)
        assert torch.equal(oview, out0) and torch.equal(hview, h0) and torch.equal(rview, x)
        for b_, v_ in ((obuf, oview), (hbuf, hview), (rbuf, rview)):
            assert_frame_intact(b_, v_)
        obuf, oview = _framed_copy(x, po)  # in place, as the decoder runs it (out=None: out is resid)
        hbuf, hview = _frame(M, N, ph)
        K.gemm_resid_norm(a, w, oview, g, 1e-5, h_out=hview, splits=splits)
        assert torch.equal(oview, out0) and torch.equal(hview, h0)
        assert_frame_intact(obuf, oview)
        assert_frame_intact(hbuf, hview)


# -------------------------------------------------------------------------- gemm_rope / rope_cache
def _cache_rows_untouched(cache, before, slot, pos):
    """Every [slot, :, pos, :] row of ``cache`` that no (slot[t], pos[t]) addresses has the bits of
    ``before``."""
    S, _, L, _ = cache.shape
    hit = torch.zeros(S, L, dtype=torch.bool, device=cache.device)
    hit[slot.long(), pos.long()] = True
    keep = ~hit
    return torch.equal(cache.transpose(1, 2)[keep], before.transpose(1, 2)[keep])


@pytest.mark.parametrize("kv_out", [True, False])
@pytest.mark.parametrize("H,Hkv,D", [(4, 4, 96), (8, 2, 128)])
def test_gemm_rope_writes(H, Hkv, D, kv_out):
    """QKV GEMM with RoPE + KV-cache write in the epilogue (M = 300: two ragged 256-row tiles): ``out``
    framed, caches started from random contents — only the (slot, pos) rows change."""
    torch.manual_seed(H + D)
    M, Kd, S, L = 300, 256, 3, 512
    N = (H + 2 * Hkv) * D
    a, w = _rand(M, Kd), _rand(N, Kd, scale=Kd ** -0.5)
    slot = torch.randint(0, S, (M,), device=DEV, dtype=torch.int32)
    pos = torch.randperm(L, device=DEV)[:M].to(torch.int32)  # unique positions: unique (slot, pos)
    cs = R.rope_table(L, D, 10000.0, device=DEV)
    kc0, vc0 = _rand(S, Hkv, L, D), _rand(S, Hkv, L, D)
    kc1, vc1 = kc0.clone(), vc0.clone()
    want = K.gemm_rope(a, w, pos, cs, H, Hkv, D, slot, kc1, vc1)  # contiguous out, kv_out=True
    kcr, vcr = kc0.clone(), vc0.clone()
    _close(want, R.gemm_rope(a, w, pos, cs, H, Hkv, D, slot, kcr, vcr), atol=0.03)
    _close(kc1, kcr, atol=0.03)
    _close(vc1, vcr, atol=0.03)
    assert _cache_rows_untouched(kc1, kc0, slot, pos) and _cache_rows_untouched(vc1, vc0, slot, pos)
    assert not torch.equal(kc1, kc0) and not torch.equal(vc1, vc0)
    for pad in PADS:
        buf, view = _frame(M, N, pad)
        kc2, vc2 = kc0.clone(), vc0.clone()
        K.gemm_rope(a, w, pos, cs, H, Hkv, D, slot, kc2, vc2, out=view, kv_out=kv_out)
        assert torch.equal(view[:, :H * D], want[:, :H * D])
        if kv_out:
            assert torch.equal(view, want)
        assert torch.equal(kc2, kc1) and torch.equal(vc2, vc1)
        assert_frame_intact(buf, view)


@pytest.mark.parametrize("rotate_q", [True, False])
@pytest.mark.parametrize("H,Hkv,D", [(4, 4, 96), (8, 2, 128)])
def test_rope_cache_writes(H, Hkv, D, rotate_q):
    """rope_cache on the same inputs: qkv (contiguous, as the wrapper requires) between guard elements,
    caches from random contents; rotate_q=False leaves the q columns bit-unchanged and rotates / stores
    the same k and v."""
    torch.manual_seed(H + D)
    M, Kd, S, L = 300, 256, 3, 512
    N = (H + 2 * Hkv) * D
    a, w = _rand(M, Kd), _rand(N, Kd, scale=Kd ** -0.5)
    slot = torch.randint(0, S, (M,), device=DEV, dtype=torch.int32)
    pos = torch.randperm(L, device=DEV)[:M].to(torch.int32)
    cs = R.rope_table(L, D, 10000.0, device=DEV)
    kc0, vc0 = _rand(S, Hkv, L, D), _rand(S, Hkv, L, D)
    raw = K.gemm(a, w)
    full, kcf, vcf = raw.clone(), kc0.clone(), vc0.clone()
    K.rope_cache(full, pos, cs, H, Hkv, D, slot=slot, k_cache=kcf, v_cache=vcf)
    ref, kcr, vcr = raw.clone(), kc0.clone(), vc0.clone()
    R.rope_cache(ref, pos, cs, H, Hkv, D, slot=slot, k_cache=kcr, v_cache=vcr)
    _close(full, ref, atol=0.02)
    _close(kcf, kcr, atol=0.02)
    _close(vcf, vcr, atol=0)
    gbuf, flat = guarded(M * N, BF16, guard=4096, device=DEV)
    qkv = flat.view(M, N)
    qkv.copy_(raw)
    kc, vc = kc0.clone(), vc0.clone()
    K.rope_cache(qkv, pos, cs, H, Hkv, D, slot=slot, k_cache=kc, v_cache=vc, rotate_q=rotate_q)
    assert_frame_intact(gbuf, flat, "qkv guards")
    assert torch.equal(qkv[:, H * D:], full[:, H * D:])
    assert torch.equal(qkv[:, :H * D], full[:, :H * D] if rotate_q else raw[:, :H * D])
    assert torch.equal(kc, kcf) and torch.equal(vc, vcf)
    assert _cache_rows_untouched(kc, kc0, slot, pos) and _cache_rows_untouched(vc, vc0, slot, pos)
    # no cache: only qkv is written
    q2 = raw.clone()
    K.rope_cache(q2, pos, cs, H, Hkv, D, rotate_q=rotate_q)
    assert torch.equal(q2, qkv)


# --------------------------------------------------------------------- fp8 / fp16 GEMMs, quantisers
@pytest.mark.parametrize("epi", [K.EPI_NONE, K.EPI_RESID])
def test_gemm_fp8_writes(epi):
    torch.manual_seed(8 + epi)
    M, N, Kd = 300, 264, 128
    x, w = _rand(M, Kd), _rand(N, Kd, scale=Kd ** -0.5)
    resid = _rand(M, N) if epi == K.EPI_RESID else None
    xq, sa = K.quant_fp8(x)
    wq, sw = K.quant_weight_fp8(w)

    def run(out, r):
        return K.gemm_fp8(xq, sa, wq, sw, epi=epi, resid=r, out=out)
    want = run(None, resid)
    _close(want, R.gemm_fp8(xq, sa, wq, sw, epi=epi, resid=resid), atol=0.03)
    _write_check(run, M, N, want, resid=resid)


@pytest.mark.parametrize("Kd", [128, 272])
@pytest.mark.parametrize("pad", [16, 48])
def test_quant_fp8_writes(pad, Kd):
    """Row quantiser: fp8 ``out`` framed (row stride a multiple of 16 bytes, so K % 16 == 0: the fp8
    GEMM's K = 128, and 272 = 34 chunks of 8, not a multiple of the 64-lane row loop), ``scale`` between
    guards, and a strided input."""
    torch.manual_seed(pad + Kd)
    M = 300
    x = _rand(M, Kd + 8)[:, :Kd]
    q0, s0 = K.quant_fp8(x)
    rq, rs = R.quant_fp8(x.contiguous())
    assert torch.allclose(s0, rs, rtol=1e-6)
    d = (q0.float() - rq.float()).abs()
    assert (d > 0).float().mean().item() < 1e-2
    assert torch.all(d <= 0.126 * rq.float().abs() + 2 ** -9)
    buf, view = _frame(M, Kd, pad, dtype=K.FP8)
    sbuf, scale = guarded(M, torch.float32, device=DEV)
    K.quant_fp8(x, out=view, scale=scale)
    assert torch.equal(view.view(torch.uint8), q0.view(torch.uint8)) and torch.equal(scale, s0)
    assert_frame_intact(buf, view, "fp8 out")
    assert_frame_intact(sbuf, scale, "scale guards")


@pytest.mark.parametrize("resid", [False, True])
def test_layernorm_fp8_out_writes(resid):
    """layernorm(fp8_out=True) allocates y / yq / ys itself; here the same library entry point writes
    into flat guarded buffers (M = 333 rows, D = 264: not a multiple of the 256-thread row loop)."""
    torch.manual_seed(11)
    M, D = 333, 264
    x, r = _rand(M, D), (_rand(M, D) if resid else None)
    g, b = _rand(D) + 1, _rand(D)
    y0, yq0, ys0 = K.layernorm(x, g, b, 1e-12, resid=r, fp8_out=True)
    ry, rq, rs = R.layernorm(x, g, b, 1e-12, resid=r, fp8_out=True)
    _close(y0, ry, atol=0.03)
    assert torch.allclose(ys0, rs, rtol=1e-3)
    d = (yq0.float() * ys0[:, None] - rq.float() * rs[:, None]).abs()
    assert torch.all(d <= 0.13 * (rq.float() * rs[:, None]).abs() + 1e-3)
    ybuf, y = guarded(M * D, BF16, guard=1024, device=DEV)
    qbuf, yq = guarded(M * D, K.FP8, guard=1024, device=DEV)
    sbuf, ys = guarded(M, torch.float32, device=DEV)
    K._check(K.lib().da_layernorm_q(K._ptr(x), K._ptr(r), K._ptr(g), K._ptr(b), K._ptr(y), K._ptr(yq), K._ptr(ys),
                                    M, D, 1e-12, K._stream()), "layernorm_q")
    assert torch.equal(y.view(M, D), y0) and torch.equal(ys, ys0)
    assert torch.equal(yq.view(torch.uint8).view(M, D), yq0.view(torch.uint8))
    for b_, v_ in ((ybuf, y), (qbuf, yq), (sbuf, ys)):
        assert_frame_intact(b_, v_)


@pytest.mark.parametrize("epi", [K.EPI_NONE, K.EPI_RESID])
def test_gemm_f16_writes(epi):
    torch.manual_seed(16 + epi)
    M, N, Kd = 300, 264, 192
    f16 = torch.float16
    a, w = _rand(M, Kd, dtype=f16), _rand(N, Kd, scale=Kd ** -0.5, dtype=f16)
    resid = _rand(M, N, dtype=f16) if epi == K.EPI_RESID else None

    def run(out, r):
        return K.gemm_f16(a, w, epi=epi, resid=r, out=out)
    want = run(None, resid)
    torch.testing.assert_close(want.float(), R.gemm_f16(a, w, epi=epi, resid=resid).float(), atol=6e-3, rtol=6e-3)
    _write_check(run, M, N, want, dtype=f16, resid=resid)


# -------------------------------------------------------------------------------- flash attention
LENS = [1, 77, 130]
FH, FHKV = 4, 2


def _cu(lens):
    return torch.tensor([0] + list(np.cumsum(lens)), device=DEV, dtype=torch.int32)


def _flash_check(run, T, D, want, dtype=BF16):
    for pad in PADS:
        buf, view = _frame(T, FH * D, pad, dtype)
        run(view)
        assert torch.equal(view, want), f"framed out (pad {pad}) differs from the contiguous launch"
        assert_frame_intact(buf, view)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [32, 64, 96, 128])
def test_flash_attn_writes(D, causal):
    """Every kernel the dispatch picks (4-wave flash_attn_v2 at D = 32 / 64 / 96, 8-wave at D = 128,
    the pipelined kernel at causal D = 96), GQA, sequences of 1 / 77 / 130 tokens (one row, a partial
    query block, one block + 2 rows)."""
    torch.manual_seed(D + causal)
    T = sum(LENS)
    q, k, v = _rand(T, FH * D), _rand(T, FHKV * D), _rand(T, FHKV * D)
    cu = _cu(LENS)

    def run(out):
        return K.flash_attn_varlen(q, k, v, cu, max(LENS), FH, FHKV, D, causal, out=out)
    want = run(None)
    _close(want, R.flash_attn_varlen(q, k, v, cu, max(LENS), FH, FHKV, D, causal), atol=0.02)
    _flash_check(run, T, D, want)


@pytest.mark.parametrize("mode", ["prefix64", "prefix40", "kv_cache", "kv_cache_prefix64"])
def test_flash_attn_d96_prefix_and_cache_writes(mode):
    """Causal D = 96: shared prefix of whole 64-key tiles (LDS-DMA pipelined kernel), a ragged prefix
    (register-staged form), and the sequences' own keys read from the KV cache; the caches and the
    prefix slot are inputs only and must come back bit-unchanged."""
    torch.manual_seed(len(mode))
    D, S, L = 96, 4, 512
    T = sum(LENS)
    cu = _cu(LENS)
    kc, vc = _rand(S, FHKV, L, D), _rand(S, FHKV, L, D)
    P = {"prefix64": 64, "prefix40": 40, "kv_cache": 0, "kv_cache_prefix64": 64}[mode]
    pre = (kc[3], vc[3], P) if P else None
    q = _rand(T, FH * D)
    slot = torch.cat([torch.full((n,), b, dtype=torch.int32) for b, n in enumerate(LENS)]).to(DEV)
    pos = torch.cat([torch.arange(P, P + n, dtype=torch.int32) for n in LENS]).to(DEV)
    # the k / v columns a packed qkv would hold: the cache rows of each token
    k = kc[slot.long(), :, pos.long()].reshape(T, FHKV * D).contiguous()
    v = vc[slot.long(), :, pos.long()].reshape(T, FHKV * D).contiguous()
    kc0, vc0 = kc.clone(), vc.clone()
    kvc = (kc, vc, slot, pos) if mode.startswith("kv_cache") else None

    def run(out):
        if kvc is not None:
            return K.flash_attn_varlen(q, None, None, cu, max(LENS), FH, FHKV, D, True, prefix=pre, kv_cache=kvc, out=out)
        return K.flash_attn_varlen(q, k, v, cu, max(LENS), FH, FHKV, D, True, prefix=pre, out=out)
    want = run(None)
    _close(want, R.flash_attn_varlen(q, k, v, cu, max(LENS), FH, FHKV, D, True, prefix=pre), atol=0.02)
    if kvc is not None:  # == the attention over the k / v columns (as test_flash_attn_kv_from_cache)
        assert torch.equal(want, K.flash_attn_varlen(q, k, v, cu, max(LENS), FH, FHKV, D, True, prefix=pre))
    _flash_check(run, T, D, want)
    assert torch.equal(kc, kc0) and torch.equal(vc, vc0)


@pytest.mark.parametrize("D,causal", [(96, True), (64, False), (64, True), (128, True)])
def test_flash_attn_tail_only_writes(D, causal):
    """tail_only on a framed ``out`` pre-filled with the pattern: per sequence only the query block
    holding its last token is stored (128 rows; 256 on the 8-wave D = 128 kernel), with the bits of a
    full launch; every other row of ``out`` and the frame still hold the pattern."""
    torch.manual_seed(D + causal + 1)
    T = sum(LENS)
    q, k, v = _rand(T, FH * D), _rand(T, FHKV * D), _rand(T, FHKV * D)
    cu = _cu(LENS)
    want = K.flash_attn_varlen(q, k, v, cu, max(LENS), FH, FHKV, D, causal)
    _close(want, R.flash_attn_varlen(q, k, v, cu, max(LENS), FH, FHKV, D, causal), atol=0.02)
    blk = 256 if D == 128 else 128
    for pad in PADS:
        buf, view = _frame(T, FH * D, pad)
        fill_pattern(view)
        K.flash_attn_varlen(q, k, v, cu, max(LENS), FH, FHKV, D, causal, out=view, tail_only=True)
        assert_frame_intact(buf, view)
        s0 = 0
        for n in LENS:
            t0 = s0 + (n - 1) // blk * blk
            assert torch.equal(view[t0:s0 + n], want[t0:s0 + n])
            assert holds_pattern(view[s0:t0]), f"rows before the last query block of the {n}-token sequence written"
            s0 += n
    assert (130 - 1) // 128 * 128 == 128  # the 130-token sequence has rows outside its last block (D != 128)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 96])
def test_flash_attn_f16_writes(D, causal):
    torch.manual_seed(D + causal + 16)
    f16 = torch.float16
    T = sum(LENS)
    q, k, v = _rand(T, FH * D, dtype=f16), _rand(T, FHKV * D, dtype=f16), _rand(T, FHKV * D, dtype=f16)
    cu = _cu(LENS)

    def run(out):
        return K.flash_attn_f16(q, k, v, cu, max(LENS), FH, FHKV, D, causal, out=out)
    want = run(None)
    ref = R.flash_attn_f16(q, k, v, cu, max(LENS), FH, FHKV, D, causal)
    torch.testing.assert_close(want.float(), ref.float(), atol=4e-3, rtol=4e-3)
    _flash_check(run, T, D, want, dtype=f16)


# ------------------------------------------------------------------------------- decode attention
DLENS = [1, 64, 65, 700]


def _decode_case(H, Hkv, D, chunk, rope):
    torch.manual_seed(H + D + chunk + rope)
    B, S, max_seq = len(DLENS), len(DLENS) + 2, 768
    width = (H + 2 * Hkv) * D
    kc0, vc0 = _rand(S, Hkv, max_seq, D), _rand(S, Hkv, max_seq, D)
    lens = torch.tensor(DLENS, dtype=torch.int32, device=DEV)
    slot = torch.tensor([4, 0, 2, 1], dtype=torch.int32, device=DEV)
    pos = lens - 1
    qkv0 = _rand(B, width)
    cs = R.rope_table(max_seq, D, 10000.0, device=DEV)
    rp = (cs, pos) if rope else None
    kc1, vc1 = kc0.clone(), vc0.clone()
    want = K.decode_attn(qkv0, kc1, vc1, lens, slot, H, Hkv, D, max_seq, chunk=chunk, rope=rp)
    _close(want, R.decode_attn(qkv0.clone(), kc0.clone(), vc0.clone(), lens, slot, H, Hkv, D, rope=rp), atol=0.02)
    for pad in PADS:
        qbuf, q = _framed_copy(qkv0, pad)  # row stride larger than (H + 2 Hkv) D
        assert q.stride(0) > width
        obuf, out = _frame(B, H * D, PADS[0] + PADS[1] - pad)
        kc, vc = kc0.clone(), vc0.clone()
        for it in range(3):  # repeated launches: the split counters must return to zero
            fill_pattern(out)
            K.decode_attn(q, kc, vc, lens, slot, H, Hkv, D, max_seq, chunk=chunk, out=out, rope=rp)
            assert torch.equal(out, want), f"launch {it} (pad {pad}) differs from the contiguous launch"
            assert_frame_intact(obuf, out)
            assert_frame_intact(qbuf, q)
            assert torch.equal(q, qkv0), "the qkv rows are inputs only"
        assert torch.equal(kc, kc1) and torch.equal(vc, vc1)
    if not rope:
        assert torch.equal(kc1, kc0) and torch.equal(vc1, vc0)
        return
    # everything except the B rows [slot[b], :, pos[b], :] is bit-identical to the clone
    assert _cache_rows_untouched(kc1, kc0, slot, pos) and _cache_rows_untouched(vc1, vc0, slot, pos)
    kcr, vcr = kc0.clone(), vc0.clone()
    R.rope_cache(qkv0.clone(), pos, cs, H, Hkv, D, slot=slot, k_cache=kcr, v_cache=vcr)
    _close(kc1, kcr, atol=0.02)
    assert torch.equal(vc1, vcr)
    assert not torch.equal(kc1, kc0)


@pytest.mark.parametrize("xc", [True, False])
@pytest.mark.parametrize("rope", [False, True])
@pytest.mark.parametrize("chunk", [64, 0])
def test_decode_attn_mha_small_batch_writes(chunk, rope, xc, monkeypatch):
    """MHA D = 96, B * Hkv = 32 (the prefetching variant): splits exchanged through one XCD's L2
    (DECODE_XC on) and through uncached memory (off)."""
    monkeypatch.setattr(K, "DECODE_XC", xc)
    assert (not xc) or K.decode_xc_ok(torch.device(DEV))
    _decode_case(8, 8, 96, chunk, rope)


@pytest.mark.parametrize("rope", [False, True])
@pytest.mark.parametrize("chunk", [64, 0])
@pytest.mark.parametrize("D", [64, 96])
def test_decode_attn_mha_streaming_writes(D, chunk, rope):
    """B * Hkv = 64 > 32: the streaming variant."""
    _decode_case(16, 16, D, chunk, rope)


@pytest.mark.parametrize("chunk", [64, 0])
@pytest.mark.parametrize("H,Hkv,D", [(8, 2, 128), (8, 2, 96), (8, 2, 64)])
def test_decode_attn_gqa_writes(H, Hkv, D, chunk):
    """GQA: the MFMA kernel (D = 128 / 64) and the VALU kernel (D = 96)."""
    _decode_case(H, Hkv, D, chunk, False)


# ---------------------------------------------------------------------------------------- sampler
def _padded_logits(B, V):
    """logits [B, V] as a view of a [B + 1, ld] buffer, ld = next multiple of 8 of V plus 8; the pad
    columns and the row after the last hold 60.0, larger than any real logit (|x| < 3 * 6): a read past
    V, or past the last row, changes the argmax and the log-sum-exp."""
    ld = (V + 7) // 8 * 8 + 8
    big = torch.full((B + 1, ld), 60.0, dtype=BF16, device=DEV)
    view = big[:B, :V]
    view.copy_(_rand(B, V, scale=3.0).clamp_(-18, 18))
    return big, view


@pytest.mark.parametrize("V", [4099, 1003])
def test_sample_reads_stay_inside_strided_rows(V):
    """sample on a strided logits view (V = 4099: chunked, V % 8 != 0, a last chunk of 3 entries;
    V = 1003: one workgroup per row with a scalar tail), the one-workgroup kernel forced at V = 4099
    too, and sample_partial + sample_finalize on two slices of the same view."""
    torch.manual_seed(V)
    B = 3
    big, logits = _padded_logits(B, V)
    copy = logits.contiguous()
    rtok, rlp = R.sample(copy.cpu(), 0.0, 1, 0)
    assert int(rtok.max()) < V and float(copy.max()) < 60.0
    assert K.SAMPLE_CHUNKED_MAX_B >= B  # V >= 4096 takes the chunked kernel

    def check(tok, lp, what):
        torch.cuda.synchronize()
        assert torch.equal(tok.cpu(), rtok), f"{what}: tokens {tok.tolist()} vs {rtok.tolist()}"
        _close(lp.cpu(), rlp, atol=2e-3)
    check(*K.sample(logits, 0.0, 1, 0), "sample")
    old = K.SAMPLE_CHUNKED_MAX_B
    try:
        K.SAMPLE_CHUNKED_MAX_B = 0
        check(*K.sample(logits, 0.0, 1, 0), "sample, one workgroup per row")
    finally:
        K.SAMPLE_CHUNKED_MAX_B = old
    V0 = V // 2 + 1  # odd split: the second slice starts on an unaligned element
    stats = torch.cat([K.sample_partial(logits[:, :V0], 0.0, 1, 0), K.sample_partial(logits[:, V0:], 0.0, 1, V0)],
                      dim=1).contiguous()
    check(*K.sample_finalize(stats, 2), "sample_partial + sample_finalize")
    assert bool((big[B] == 60.0).all()) and bool((big[:B, V:] == 60.0).all())  # inputs only


EOS = (5, 9, 13, 17, 21)  # a fifth id is passed and must be ignored (the kernels take four)
HIST_LD = 8
BK_B, BK_V = 12, 4096
# row -> (active, start, pos, spike token at steps 0..2)
BK_ROWS = [
    (0, 10, 12, (100, 101, 102)),    # inactive from the start: every output keeps its pre-filled value
    (1, 10, 12, (5, 111, 112)),      # EOS at step 0: active clears, pos / lens advance, token in hist
    (1, 10, 17, (120, 121, 122)),    # pos - start == hist_ld - 1: last slot written, history full -> stop
    (1, 10, 18, (130, 131, 132)),    # pos - start == hist_ld: nothing stored, stop
    (1, 20, 18, (140, 141, 142)),    # pos < start: negative index, nothing stored until step 2 (index 0)
    (1, 10, 11, (150, 17, 152)),     # the fourth EOS id at step 1
    (1, 10, 11, (21, 161, 162)),     # the fifth id: not an EOS, the row goes on
    (1, 10, 10, (170, 171, 9)),      # the second EOS id at step 2
    (1, 10, 15, (180, 181, 182)),    # fills hist[5], [6], [7]: stops only at step 2
    (1, 10, 10, (190, 191, 192)),    # plain active rows
    (1, 0, 3, (4000, 4095, 0)),
    (1, 7, 9, (1023, 1024, 2048)),
]


def _bk_logits():
    torch.manual_seed(77)
    steps = []
    for s in range(3):
        x = torch.randn(BK_B, BK_V) * 2.0
        for b, row in enumerate(BK_ROWS):
            x[b, row[3][s]] = 30.0  # a unique spike per row: exact, tie-free tokens at T = 0
        steps.append(x.to(BF16))
    return steps


def _bk_state(device, guard):
    """The sampler's state tensors (pre-filled so an untouched entry is recognisable), each between
    guard elements when ``guard``; returns (views, buffers)."""
    init = dict(out_tok=torch.full((BK_B,), -7, dtype=torch.int32), out_lp=torch.full((BK_B,), 0.25),
                conf=torch.tensor([[0.5, 2.0]] * BK_B),
                active=torch.tensor([r[0] for r in BK_ROWS], dtype=torch.int32),
                pos=torch.tensor([r[2] for r in BK_ROWS], dtype=torch.int32),
                lens=torch.tensor([r[2] + 1 for r in BK_ROWS], dtype=torch.int32),
                hist=torch.full((BK_B, HIST_LD), -1, dtype=torch.int32),
                start=torch.tensor([r[1] for r in BK_ROWS], dtype=torch.int32))
    views, bufs = {}, {}
    for k, t in init.items():
        if guard:
            bufs[k], flat = guarded(t.numel(), t.dtype, device=device)
            views[k] = flat.view(t.shape)
            views[k].copy_(t)
        else:
            views[k] = t.clone().to(device)
    return views, bufs


_BK_REF = {}


def _bk_reference():
    """R.sample on the CPU, three steps: the whole state after each (computed once, then shared)."""
    if not _BK_REF:
        st, _ = _bk_state("cpu", False)
        snaps = []
        for s, x in enumerate(_bk_logits()):
            R.sample(x, 0.0, 3, s, eos=EOS, **st)
            snaps.append({k: v.clone() for k, v in st.items()})
        _BK_REF["snaps"] = snaps
    return _BK_REF["snaps"]


@pytest.mark.parametrize("entry", ["one_workgroup", "chunked", "partial_finalize"])
def test_sampler_bookkeeping_matches_reference(entry):
    """sample_bookkeep (shared by the one-workgroup, chunked and partial + finalize samplers) against
    R.sample's model of it, the whole state after each of three consecutive steps."""
    snaps = _bk_reference()
    st, bufs = _bk_state(DEV, True)
    old = K.SAMPLE_CHUNKED_MAX_B
    try:
        K.SAMPLE_CHUNKED_MAX_B = 0 if entry == "one_workgroup" else 64
        for s, x in enumerate(_bk_logits()):
            x = x.to(DEV)
            if entry == "partial_finalize":
                half = BK_V // 2
                stats = torch.cat([K.sample_partial(x[:, :half], 0.0, 3, 0, step=s),
                                   K.sample_partial(x[:, half:], 0.0, 3, half, step=s)], dim=1).contiguous()
                fin = {k: v for k, v in st.items()}
                K.sample_finalize(stats, 2, eos=EOS, **fin)
            else:
                K.sample(x, 0.0, 3, s, eos=EOS, **st)
            torch.cuda.synchronize()
            want = snaps[s]
            for k in ("out_tok", "active", "pos", "lens", "hist", "start"):
                assert torch.equal(st[k].cpu(), want[k]), f"step {s} {k}: {st[k].tolist()} vs {want[k].tolist()}"
            _close(st["out_lp"].cpu(), want["out_lp"], atol=2e-3, rtol=0)
            _close(st["conf"][:, 0].cpu(), want["conf"][:, 0], atol=2e-3, rtol=0)
            assert torch.equal(st["conf"][:, 1].cpu(), want["conf"][:, 1])
            for k, b_ in bufs.items():
                assert_frame_intact(b_, st[k].view(-1), f"step {s} {k} guards")
    finally:
        K.SAMPLE_CHUNKED_MAX_B = old


def test_sampler_bookkeeping_reference_row_classes():
    """The reference trace itself shows each row class (so the comparison above is about them)."""
    s0, s1, s2 = _bk_reference()
    init, _ = _bk_state("cpu", False)
    for snap in (s0, s1, s2):  # inactive row: nothing changes, out_tok and conf included
        for k in init:
            assert torch.equal(snap[k][0], init[k][0]), k
    assert s0["active"].tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1]
    assert s1["active"].tolist() == [0, 0, 0, 0, 1, 0, 1, 1, 1, 1, 1, 1]
    assert s2["active"].tolist() == [0, 0, 0, 0, 1, 0, 1, 0, 0, 1, 1, 1]
    assert s0["pos"][1] == 13 and s0["lens"][1] == 14 and s0["hist"][1, 2] == 5 and s2["pos"][1] == 13
    assert s0["hist"][2, 7] == 120 and s2["hist"][2].tolist() == [-1] * 7 + [120]
    assert s2["hist"][3].tolist() == [-1] * 8 and s0["pos"][3] == 19 and s0["out_tok"][3] == 130
    assert s1["hist"][4].tolist() == [-1] * 8 and s2["hist"][4].tolist() == [142] + [-1] * 7
    assert s1["out_tok"][5] == 17 and s2["out_tok"][5] == 17 and s2["pos"][5] == 13
    assert s2["out_tok"][6] == 162 and s2["hist"][6, 1:4].tolist() == [21, 161, 162]
    assert s2["hist"][8, 5:].tolist() == [180, 181, 182] and s1["active"][8] == 1
    assert s2["conf"][9, 1] == 5.0 and s2["conf"][0, 1] == 2.0
