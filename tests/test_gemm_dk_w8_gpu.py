"""gemm_dk on fp8 (e4m3) weights (csrc/gemm_dk_w8.hip) vs the fp32 reference on the same quantised
values, vs the bf16 gemm_dk on the dequantised matrix (bit for bit), the deferred-norm chain, what it
writes, and its refusals."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from docagents_amd.ops import kernels as K  # noqa: E402
from docagents_amd.ops import reference as R  # noqa: E402

from kernel_frames import assert_frame_intact, framed, guarded  # noqa: E402

DEV = "cuda"
# one k-chunk (shorter than the prefetch ring), BN 16; SwiGLU BN 32; SwiGLU BN 64 with a ragged last
# tile (12320 % 64 == 32); BN 16 long rows; BN 64 at 144 tiles (the fp8 rule; gemm_dk: BN 32); BN 16 at
# K = 8192; BN 64 with a ragged last tile; and, beyond the issue's list, BN 32 without SwiGLU with a
# ragged last tile (6160 = 192 x 32 + 16). Then the edges of the body the two kernels share: one tile
# and three tiles of 16 / of 32 (SwiGLU) at K = 768 (three chunks: no multiple of either prefetch depth)
# and K = 2048, the ragged 64-wide SwiGLU tile at one chunk, and a ragged 64-wide tile by the fp8 rule
# alone (9248 = 144 x 64 + 32)
PRODUCTS = [(512, 256, K.EPI_BIAS), (1024, 512, K.EPI_SWIGLU), (12320, 512, K.EPI_SWIGLU), (3072, 3072, K.EPI_RESID),
            (9216, 3072, K.EPI_NONE), (3072, 8192, K.EPI_RESID), (32064, 3072, K.EPI_NONE), (6160, 512, K.EPI_NONE),
            (16, 768, K.EPI_NONE), (48, 2048, K.EPI_RESID), (32, 768, K.EPI_SWIGLU), (96, 2048, K.EPI_SWIGLU),
            (12320, 256, K.EPI_SWIGLU), (9248, 768, K.EPI_NONE)]
ROWS = [2, 16, 17, 32]


def _rand(*shape, scale=1.0, dtype=torch.bfloat16):
    return (torch.randn(*shape, device=DEV) * scale).to(dtype)


def _close(a, b, atol, rtol=0.02):
    a, b = a.float(), b.float()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = (err > tol).sum().item()
    print(f"max err {err.max().item():.4g}, max err / tol {(err / tol).max().item():.3g}")
    assert bad == 0, f"{bad} / {a.numel()} mismatches, max err {err.max().item():.4g}"
    assert a.shape == b.shape


def _operands(M, N, Kd, epi):
    torch.manual_seed(M * 7 + N + Kd + epi)
    q, s = K.quant_weight_fp8_pow2(_rand(N, Kd, scale=Kd ** -0.5))
    return (_rand(M, Kd), q, s, _rand(N) if epi == K.EPI_BIAS else None,
            _rand(M, N) if epi == K.EPI_RESID else None)


@pytest.mark.parametrize("N,Kd,epi", PRODUCTS)
@pytest.mark.parametrize("M", ROWS)
def test_gemm_dk_w8_vs_fp32_reference(M, N, Kd, epi):
    """R.gemm_dk_w8 holds the same quantised values: only the summation order and the final bf16
    rounding differ, so test_gemm_dk_matches_reference's tolerance applies (atol 0.03, rtol 0.02)."""
    a, q, s, bias, resid = _operands(M, N, Kd, epi)
    kw = dict(epi=epi, bias=bias, resid=resid)
    got = K.gemm_dk_w8(a, q, s, **kw)
    assert got.shape == (M, N // 2 if epi == K.EPI_SWIGLU else N) and got.dtype == torch.bfloat16
    _close(got, R.gemm_dk_w8(a, q, s, **kw), atol=0.03)
    # arbitrary fp32 row scales
    s2 = (s * (0.5 + 1.5 * torch.rand(N, device=DEV))).contiguous()
    _close(K.gemm_dk_w8(a, q, s2, **kw), R.gemm_dk_w8(a, q, s2, **kw), atol=0.03)


@pytest.mark.parametrize("N,Kd,epi", PRODUCTS)
@pytest.mark.parametrize("M", ROWS)
def test_gemm_dk_w8_equals_bf16_gemm_dk_on_dequantised_weights(M, N, Kd, epi):
    """The codes are unpacked to bf16 on the way into LDS and everything after is gemm_dk_kernel's
    MFMA sequence and summation order (the k order does not depend on the tile width); a power-of-two
    row scale on the finished fp32 sum is exact. So the result is gemm_dk's on the dequantised
    matrix bit for bit: torch.equal, not a tolerance."""
    a, q, s, bias, resid = _operands(M, N, Kd, epi)
    dq = (q.float() * s[:, None]).to(torch.bfloat16)
    assert torch.equal(dq.float(), q.float() * s[:, None])
    got = K.gemm_dk_w8(a, q, s, epi=epi, bias=bias, resid=resid)
    assert torch.equal(got, K.gemm_dk(a, dq, epi=epi, bias=bias, resid=resid))


@pytest.mark.parametrize("M", [3, 16, 32])
@pytest.mark.parametrize("H,F", [(1024, 1024), (3072, 8192), (768, 1024), (2048, 1024)])
def test_gemm_dk_w8_deferred_norm_chain(M, H, F):
    """Producer (EPI_RESID + per-part sums of squares) -> consumer (deferred RMSNorm of its A rows)
    == residual add, rmsnorm kernel, reference GEMM; the sums match the fp32 row sums
    (test_gemm_dk_deferred_norm_chain's tolerances)."""
    torch.manual_seed(M + H)
    a, x = _rand(M, H), _rand(M, H)
    qo, so = K.quant_weight_fp8_pow2(_rand(H, H, scale=H ** -0.5))
    qg, sg = K.quant_weight_fp8_pow2(_rand(2 * F, H, scale=H ** -0.5))
    x_ref = x.clone()
    ssq = torch.zeros(512 * 64, dtype=torch.float32, device=DEV)
    parts = K.dk_parts(H, M)
    assert parts == K.lib().da_gemm_dk_parts(H) <= 512  # a residual producer tiles like gemm_dk's
    K.gemm_dk_w8(a, qo, so, epi=K.EPI_RESID, resid=x, out=x, ssq_out=ssq)
    _close(x, R.gemm_w8(a, qo, so, epi=K.EPI_RESID, resid=x_ref), atol=0.03)
    sums = ssq.view(-1, 64)[:parts, :M].sum(0)
    _close(sums, x.float().pow(2).sum(-1), atol=1e-2 * H, rtol=1e-3)
    g = K.gemm_dk_w8(x, qg, sg, epi=K.EPI_SWIGLU, norm_in=(ssq, parts, 1e-5))
    h = K.rmsnorm(x, torch.ones(H, dtype=torch.bfloat16, device=DEV), 1e-5)
    _close(g, R.gemm_w8(h, qg, sg, epi=K.EPI_SWIGLU), atol=0.03)
    # R.gemm_dk_w8 (the CPU model path) agrees with the kernel on both
    ssq_r = torch.zeros_like(ssq)
    x2 = x_ref.clone()
    R.gemm_dk_w8(a, qo, so, epi=K.EPI_RESID, resid=x2, out=x2, ssq_out=ssq_r)
    _close(ssq_r.view(-1, 64)[:parts, :M], ssq.view(-1, 64)[:parts, :M], atol=0.5, rtol=2e-2)
    _close(R.gemm_dk_w8(x, qg, sg, epi=K.EPI_SWIGLU, norm_in=(ssq, parts, 1e-5)), g, atol=0.03)


def test_gemm_dk_w8_in_place_residual():
    torch.manual_seed(5)
    M, N, Kd = 17, 3072, 1024
    q, s = K.quant_weight_fp8_pow2(_rand(N, Kd, scale=Kd ** -0.5))
    a, resid = _rand(M, Kd), _rand(M, N)
    want = R.gemm_dk_w8(a, q, s, epi=K.EPI_RESID, resid=resid)
    x = resid.clone()
    out = K.gemm_dk_w8(a, q, s, epi=K.EPI_RESID, resid=x, out=x)  # the decoder's x += a W^T
    assert out.data_ptr() == x.data_ptr()
    _close(x, want, atol=0.03)


@pytest.mark.parametrize("N", [48, 1056, 12320])
@pytest.mark.parametrize("M", [3, 17])
def test_gemm_dk_w8_writes_only_its_outputs(M, N):
    """Framed out with padded row strides (and a framed resid of another stride), guarded ssq_out: a
    ragged last tile at every width (N = 48: BN 16 x 3; SwiGLU 1056 % 64 == 32; 12320: BN 64, ragged),
    ragged M in the 16- and the 32-row block. Bit-identical to the contiguous launch; every byte outside
    out[:M] and the first parts * 64 floats keeps its pattern."""
    Kd = 512
    for epi in (K.EPI_NONE, K.EPI_RESID, K.EPI_SWIGLU):
        if epi == K.EPI_SWIGLU and N % 32:
            continue
        torch.manual_seed(M * 7 + N + epi)
        q, s = K.quant_weight_fp8_pow2(_rand(N, Kd, scale=Kd ** -0.5))
        a = _rand(M, Kd)
        resid = _rand(M, N) if epi == K.EPI_RESID else None
        nout = N // 2 if epi == K.EPI_SWIGLU else N
        want = K.gemm_dk_w8(a, q, s, epi=epi, resid=resid)
        _close(want, R.gemm_dk_w8(a, q, s, epi=epi, resid=resid), atol=0.03)
        for pad, rpad in ((8, 56), (24, 40)):
            buf, view = framed(M, nout, torch.bfloat16, pad, device=DEV)
            rbuf = rview = None
            if resid is not None:
                rbuf, rview = framed(M, N, torch.bfloat16, rpad, device=DEV)
                rview.copy_(resid)
            sbuf = ssq = None
            if epi == K.EPI_RESID:
                parts = K.dk_parts(N, M)
                sbuf, ssq = guarded(parts * 64, torch.float32, guard=256, device=DEV)
            got = K.gemm_dk_w8(a, q, s, epi=epi, resid=rview, out=view, ssq_out=ssq)
            assert got.data_ptr() == view.data_ptr()
            assert torch.equal(view, want), f"framed out (pad {pad}) differs from the contiguous launch"
            assert_frame_intact(buf, view, f"out pad {pad}")
            if resid is not None:
                assert_frame_intact(rbuf, rview, "resid frame")
                assert torch.equal(rview, resid), "out-of-place resid was modified"
                assert_frame_intact(sbuf, ssq, "ssq_out guards")
                sums = ssq.view(parts, 64)[:, :M].sum(0)
                _close(sums, want.float().pow(2).sum(-1), atol=1e-2 * N, rtol=1e-3)


def test_gemm_dk_w8_refusals(monkeypatch):
    """Anything the kernel would refuse raises ValueError on the host; nothing is launched."""
    def no_launch(*a, **kw):
        raise AssertionError("da_gemm_dk_w8 launched")
    a = _rand(4, 512)
    q, s = K.quant_weight_fp8_pow2(_rand(64, 512))
    x = _rand(4, 64)
    ssq = torch.zeros(512 * 64, dtype=torch.float32, device=DEV)
    K.gemm_dk_w8(a, q, s)  # accepted
    monkeypatch.setattr(K, "lib", lambda: type("L", (), {"da_gemm_dk_w8": staticmethod(no_launch)})())
    with pytest.raises(ValueError):
        K.gemm_dk_w8(_rand(33, 512), q, s)                                    # M = 33
    q3, s3 = K.quant_weight_fp8_pow2(_rand(64, 384))
    with pytest.raises(ValueError):
        K.gemm_dk_w8(_rand(4, 384), q3, s3)                                   # K % 256
    with pytest.raises(ValueError):
        K.gemm_dk_w8(a, q[:24], s[:24].contiguous())                          # N % 16
    with pytest.raises(ValueError):
        K.gemm_dk_w8(a, q[:48], s[:48].contiguous(), epi=K.EPI_SWIGLU)        # SwiGLU with N % 32
    with pytest.raises(ValueError):
        K.gemm_dk_w8(a, _rand(64, 512), s)                                    # bf16 wq
    q2, _ = K.quant_weight_fp8_pow2(_rand(64, 1024))
    with pytest.raises(ValueError):
        K.gemm_dk_w8(a, q2[:, :512], s)                                       # non-contiguous wq
    with pytest.raises(ValueError):
        K.gemm_dk_w8(a, q, s[:32])                                            # short sw
    with pytest.raises(ValueError):
        K.gemm_dk_w8(a, q, s, ssq_out=ssq)                                    # ssq_out without the residual epilogue
    with pytest.raises(ValueError):
        K.gemm_dk_w8(a, q, s, epi=K.EPI_RESID, resid=x, norm_in=(ssq, 4, 1e-5))  # deferred norm on a producer
    with pytest.raises(ValueError):
        K.gemm_dk_w8(a, q, s, out=_rand(4, 32))                               # out of another shape
    assert not K.dk_w8_fusable(33, 64, 512) and not K.dk_w8_fusable(1, 64, 512) and K.dk_w8_fusable(2, 64, 512)
    assert K.dk_w8_fusable(32, 64, 512) and not K.dk_w8_fusable(4, 64, 384) and not K.dk_w8_fusable(4, 24, 512)
    assert not K.dk_w8_fusable(4, 48, 512, K.EPI_SWIGLU) and K.dk_w8_fusable(4, 64, 512, K.EPI_SWIGLU)
    assert not K.dk_w8_fusable(4, 64, 512, K.EPI_GELU)
