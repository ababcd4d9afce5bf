"""The 33..128-row decode products on fp8 (e4m3) weights (csrc/gemm_tile_w8.hip + the *_w8 entry
points of csrc/gemm.hip): gemm_tile_w8, gemm_dk_splitk_w8 and gemm_resid_norm_w8 against the bf16 op
of the same shape on the dequantised matrix (bit for bit), against the fp32 reference, what they
write, and their refusals."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from docagents_amd.ops import gemm_plan as P  # noqa: E402
from docagents_amd.ops import kernels as K  # noqa: E402
from docagents_amd.ops import reference as R  # noqa: E402

from kernel_frames import assert_frame_intact, framed, guarded  # noqa: E402

DEV = "cuda"
ROWS = [33, 64, 65, 100, 128]
# (N, K, epi). A partial last column tile on both tiles (136 = 128 + 8 = 2 x 64 + 8; 72 = 64 + 8), with
# K = 64: one k-tile, fewer than the prefetch depth; N >= 8192 at K = 256: the unsplit 64x128 route at
# 65..128 rows (33..64 rows: the split-K hand-off at 2 splits); 9216 x 3072: three splits at 33..64 rows;
# 1024 x 1024: the 128x64 tile at 4 splits above 64 rows; every epilogue.
TILE_PRODUCTS = [(136, 256, K.EPI_NONE), (72, 64, K.EPI_BIAS), (8192, 256, K.EPI_SWIGLU), (9216, 3072, K.EPI_NONE),
                 (1024, 1024, K.EPI_RESID), (8200, 256, K.EPI_RESID), (96, 64, K.EPI_SWIGLU), (1056, 512, K.EPI_SWIGLU)]
# gemm_dk's contract: K % 256 == 0, N % 16 == 0. 144 = 128 + 16: a partial last column tile.
DK_PRODUCTS = [(144, 256, K.EPI_NONE), (512, 256, K.EPI_BIAS), (1056, 512, K.EPI_SWIGLU), (1024, 256, K.EPI_RESID),
               (9216, 3072, K.EPI_NONE), (144, 768, K.EPI_RESID)]
DK_ROWS = [33, 64]
NORM_PRODUCTS = [(136, 256), (72, 64), (1024, 1024), (3072, 512)]


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


_CACHE = {}


def _weights(N, Kd, spread=True):
    """(codes, scales, dequantised bf16 matrix) of an [N, Kd] weight whose rows were multiplied by
    2^-6 .. 2^6 before quantising: a dropped or misindexed scale is off by a power of two.
    spread=False: rows of one magnitude, for the comparisons of a deferred row norm with the fp32
    reference (the reference rounds the normalised row to bf16, the reduce scales the fp32 sum: on a
    cancelling gate sum times an up value of 64 that legitimate difference passes the tolerance, which
    tests/test_gemm_dk_w8_gpu.py states for rows of magnitude 1)."""
    if (N, Kd, spread) not in _CACHE:
        g = torch.Generator(device=DEV).manual_seed(N * 31 + Kd)
        w = torch.randn(N, Kd, device=DEV, generator=g) * Kd ** -0.5
        if spread:
            w = w * torch.exp2(torch.randint(-6, 7, (N, 1), device=DEV, generator=g).float())
        q, s = K.quant_weight_fp8_pow2(w.to(torch.bfloat16))
        dq = (q.float() * s[:, None]).to(torch.bfloat16)
        assert torch.equal(dq.float(), q.float() * s[:, None]) and (not spread or s.unique().numel() >= 4)
        _CACHE[(N, Kd, spread)] = (q, s, dq)
    return _CACHE[(N, Kd, spread)]


def _operands(M, N, Kd, epi):
    torch.manual_seed(M * 7 + N + Kd + epi)
    return (_rand(M, Kd), _rand(N) if epi in (K.EPI_BIAS, K.EPI_RESID) else None,
            _rand(M, N) if epi == K.EPI_RESID else None)


@pytest.mark.parametrize("N,Kd,epi", TILE_PRODUCTS)
@pytest.mark.parametrize("M", ROWS)
def test_gemm_tile_w8_equals_gemm_and_matches_reference(M, N, Kd, epi):
    """Bit for bit gemm() on the dequantised matrix (the same tile, split count and reduce; a power-of-two
    column scale on the fp32 value commutes with every rounding), and within test_gemm_dk_w8_gpu's
    tolerance of the fp32 reference on the same quantised values (atol 0.03, rtol 0.02)."""
    q, s, dq = _weights(N, Kd)
    a, bias, resid = _operands(M, N, Kd, epi)
    kw = dict(epi=epi, bias=bias, resid=resid)
    got = K.gemm_tile_w8(a, q, s, **kw)
    assert got.shape == (M, N // 2 if epi == K.EPI_SWIGLU else N) and got.dtype == torch.bfloat16
    assert torch.equal(got, K.gemm(a, dq, **kw))
    _close(got, R.gemm_tile_w8(a, q, s, **kw), atol=0.03)
    if epi == K.EPI_RESID:  # in place: the decoder's x += a W^T
        x = resid.clone()
        assert K.gemm_tile_w8(a, q, s, epi=epi, bias=bias, resid=x, out=x).data_ptr() == x.data_ptr()
        assert torch.equal(x, got)


def test_tile_products_cover_the_routes():
    """The shapes above reach every launch form: both tiles, one split and several, three splits."""
    seen = set()
    for M in ROWS:
        for N, Kd, epi in TILE_PRODUCTS:
            p = P.plan_tile_w8(M, N, Kd, epi, cus=256)
            seen.add((p.tile, min(p.splits, 5)))
    assert {(2, 1), (2, 2), (2, 3), (9, 1), (9, 4)} <= seen, seen


@pytest.mark.parametrize("N,Kd,epi", DK_PRODUCTS)
@pytest.mark.parametrize("M", DK_ROWS)
def test_gemm_dk_splitk_w8_equals_gemm_dk_and_matches_reference(M, N, Kd, epi):
    q, s, dq = _weights(N, Kd)
    a, bias, resid = _operands(M, N, Kd, epi)
    kw = dict(epi=epi, bias=bias, resid=resid)
    got = K.gemm_dk_splitk_w8(a, q, s, **kw)
    assert torch.equal(got, K.gemm_dk(a, dq, **kw))
    _close(got, R.gemm_dk_splitk_w8(a, q, s, **kw), atol=0.03)
    if epi != K.EPI_RESID:  # the deferred row norm in the reduce
        ssq = (torch.rand(4 * 64, device=DEV) * Kd).contiguous()
        got = K.gemm_dk_splitk_w8(a, q, s, norm_in=(ssq, 4, 1e-5), **kw)
        assert torch.equal(got, K.gemm_dk(a, dq, norm_in=(ssq, 4, 1e-5), **kw))
        q1, s1, _ = _weights(N, Kd, spread=False)
        _close(K.gemm_dk_splitk_w8(a, q1, s1, norm_in=(ssq, 4, 1e-5), **kw),
               R.gemm_dk_splitk_w8(a, q1, s1, norm_in=(ssq, 4, 1e-5), **kw), atol=0.03)
    else:
        x = resid.clone()
        assert K.gemm_dk_splitk_w8(a, q, s, epi=epi, bias=bias, resid=x, out=x).data_ptr() == x.data_ptr()
        assert torch.equal(x, K.gemm_dk(a, dq, **kw))


@pytest.mark.parametrize("M", DK_ROWS)
@pytest.mark.parametrize("H,F", [(1024, 512), (3072, 1024)])
def test_gemm_dk_splitk_w8_row_sums_chain(M, H, F):
    """A residual producer with ssq_out (N % 512 == 0: one part per 512 columns) and the consumer that
    takes those sums as its deferred norm: out and ssq_out equal gemm_dk's bit for bit, and the chain
    matches residual add, rmsnorm kernel, reference product."""
    torch.manual_seed(M + H)
    qo, so, dqo = _weights(H, H)
    qg, sg, dqg = _weights(2 * F, H)
    a, x0 = _rand(M, H), _rand(M, H)
    parts = K.dk_parts(H, M)
    assert parts == H // 512
    ssq8 = torch.zeros(parts * 64, dtype=torch.float32, device=DEV)
    ssq = torch.zeros_like(ssq8)
    x8, x = x0.clone(), x0.clone()
    K.gemm_dk_splitk_w8(a, qo, so, epi=K.EPI_RESID, resid=x8, out=x8, ssq_out=ssq8)
    K.gemm_dk(a, dqo, epi=K.EPI_RESID, resid=x, out=x, ssq_out=ssq)
    assert torch.equal(x8, x) and torch.equal(ssq8, ssq)
    _close(x8, R.gemm_tile_w8(a, qo, so, epi=K.EPI_RESID, resid=x0), atol=0.03)
    _close(ssq8.view(parts, 64)[:, :M].sum(0), x8.float().pow(2).sum(-1), atol=1e-2 * H, rtol=1e-3)
    g8 = K.gemm_dk_splitk_w8(x8, qg, sg, epi=K.EPI_SWIGLU, norm_in=(ssq8, parts, 1e-5))
    assert torch.equal(g8, K.gemm_dk(x, dqg, epi=K.EPI_SWIGLU, norm_in=(ssq, parts, 1e-5)))
    h = K.rmsnorm(x8, torch.ones(H, dtype=torch.bfloat16, device=DEV), 1e-5)
    q1, s1, _ = _weights(2 * F, H, spread=False)
    _close(K.gemm_dk_splitk_w8(x8, q1, s1, epi=K.EPI_SWIGLU, norm_in=(ssq8, parts, 1e-5)),
           R.gemm_tile_w8(h, q1, s1, epi=K.EPI_SWIGLU), atol=0.03)


@pytest.mark.parametrize("N,Kd", NORM_PRODUCTS)
@pytest.mark.parametrize("M", ROWS)
def test_gemm_resid_norm_w8_equals_gemm_resid_norm_and_matches_reference(M, N, Kd):
    q, s, dq = _weights(N, Kd)
    torch.manual_seed(M + N + Kd)
    a, x0, gamma, bias = _rand(M, Kd), _rand(M, N), (1 + 0.1 * _rand(N).float()).to(torch.bfloat16), _rand(N)
    for b in (None, bias):
        x8, x, xr = x0.clone(), x0.clone(), x0.clone()  # in place: out is resid
        h8 = K.gemm_resid_norm_w8(a, q, s, x8, gamma, 1e-5, bias=b)
        h = K.gemm_resid_norm(a, dq, x, gamma, 1e-5, bias=b)
        assert torch.equal(x8, x) and torch.equal(h8, h) and not torch.equal(x8, x0)
        hr = R.gemm_resid_norm_w8(a, q, s, xr, gamma, 1e-5, bias=b)
        _close(x8, xr, atol=0.03)
        _close(h8, hr, atol=0.03)
    out, h_out = torch.empty_like(x0), torch.empty_like(x0)  # out of place
    K.gemm_resid_norm_w8(a, q, s, x0, gamma, 1e-5, out=out, h_out=h_out, bias=bias)
    assert torch.equal(out, x8) and torch.equal(h_out, h8)


def _framed_workspace(monkeypatch):
    """kernels._workspace replaced by one that hands out exactly the bytes asked for, inside guards."""
    made = []

    def ws(nbytes, device):
        buf, view = guarded(nbytes, torch.uint8, guard=4096, device=DEV)
        made.append((buf, view))
        return view
    monkeypatch.setattr(K, "_workspace", ws)
    return made


@pytest.mark.parametrize("M", [33, 100])
def test_ops_write_only_their_outputs(M, monkeypatch):
    """Padded row strides and pattern frames around out, h_out, ssq_out and the split-K workspace, a
    partial last column tile (136 on the tile ops, 1040 = 8 x 128 + 16 on the dk route), ragged M in the
    last row block: bit-identical to the contiguous launch, every byte outside the outputs untouched."""
    Kd = 512
    for epi, N in ((K.EPI_NONE, 136), (K.EPI_RESID, 136), (K.EPI_SWIGLU, 1056)):
        q, s, _ = _weights(N, Kd)
        a, bias, resid = _operands(M, N, Kd, epi)
        nout = N // 2 if epi == K.EPI_SWIGLU else N
        want = K.gemm_tile_w8(a, q, s, epi=epi, bias=bias, resid=resid)
        for pad, rpad in ((8, 56), (24, 40)):
            made = _framed_workspace(monkeypatch)
            buf, view = framed(M, nout, torch.bfloat16, pad, device=DEV)
            rbuf = rview = None
            if resid is not None:
                rbuf, rview = framed(M, N, torch.bfloat16, rpad, device=DEV)
                rview.copy_(resid)
            K.gemm_tile_w8(a, q, s, epi=epi, bias=bias, resid=rview, out=view)
            assert torch.equal(view, want)
            assert_frame_intact(buf, view, f"gemm_tile_w8 out pad {pad}")
            for wbuf, wview in made:
                assert_frame_intact(wbuf, wview, "gemm_tile_w8 workspace")
            if resid is not None:
                assert_frame_intact(rbuf, rview, "resid frame")
                assert torch.equal(rview, resid)
            monkeypatch.undo()
    # gemm_resid_norm_w8: out, h_out and the workspace
    N = 136
    q, s, _ = _weights(N, Kd)
    torch.manual_seed(M)
    a, x0, gamma = _rand(M, Kd), _rand(M, N), _rand(N)
    want_x = x0.clone()
    want_h = K.gemm_resid_norm_w8(a, q, s, want_x, gamma, 1e-5)
    for pad, hpad in ((8, 56), (24, 40)):
        made = _framed_workspace(monkeypatch)
        xbuf, xview = framed(M, N, torch.bfloat16, pad, device=DEV)
        hbuf, hview = framed(M, N, torch.bfloat16, hpad, device=DEV)
        xview.copy_(x0)
        K.gemm_resid_norm_w8(a, q, s, xview, gamma, 1e-5, h_out=hview)
        assert torch.equal(xview, want_x) and torch.equal(hview, want_h)
        assert_frame_intact(xbuf, xview, "gemm_resid_norm_w8 out")
        assert_frame_intact(hbuf, hview, "gemm_resid_norm_w8 h_out")
        assert len(made) == 1
        assert_frame_intact(made[0][0], made[0][1], "gemm_resid_norm_w8 workspace")
        monkeypatch.undo()
    if M > K.DK_MAX_M:
        return
    # gemm_dk_splitk_w8: out, ssq_out and the workspace
    for epi, N in ((K.EPI_NONE, 1040), (K.EPI_RESID, 1024)):
        q, s, _ = _weights(N, Kd)
        a, bias, resid = _operands(M, N, Kd, epi)
        ssq_want = torch.zeros(K.dk_parts(N, M) * 64, dtype=torch.float32, device=DEV) if epi == K.EPI_RESID else None
        want = K.gemm_dk_splitk_w8(a, q, s, epi=epi, bias=bias, resid=resid, ssq_out=ssq_want)
        made = _framed_workspace(monkeypatch)
        buf, view = framed(M, N, torch.bfloat16, 24, device=DEV)
        sbuf = ssq = None
        if epi == K.EPI_RESID:
            sbuf, ssq = guarded(K.dk_parts(N, M) * 64, torch.float32, guard=256, device=DEV)
        K.gemm_dk_splitk_w8(a, q, s, epi=epi, bias=bias, resid=resid, out=view, ssq_out=ssq)
        assert torch.equal(view, want)
        assert_frame_intact(buf, view, "gemm_dk_splitk_w8 out")
        assert len(made) == 1
        assert_frame_intact(made[0][0], made[0][1], "gemm_dk_splitk_w8 workspace")
        if ssq is not None:
            assert_frame_intact(sbuf, ssq, "ssq_out guards")
            parts = K.dk_parts(N, M)
            assert torch.equal(ssq.view(parts, 64)[:, :M], ssq_want.view(parts, 64)[:, :M])
            # rows M .. 63 of a part are not this launch's
            assert bool((ssq.view(parts, 64)[:, M:].view(torch.int32) == 0x5A5A5A5A).all())
        monkeypatch.undo()


def test_refusals(monkeypatch):
    """Anything the kernels would refuse raises ValueError on the host; nothing is launched."""
    def no_launch(*a, **kw):
        raise AssertionError("launched")
    N, Kd = 64, 512
    q, s, _ = _weights(N, Kd)
    a, x, gamma = _rand(40, Kd), _rand(40, N), _rand(N)
    ssq = torch.zeros(512 * 64, dtype=torch.float32, device=DEV)
    K.gemm_tile_w8(a, q, s), K.gemm_dk_splitk_w8(a, q, s), K.gemm_resid_norm_w8(a, q, s, x.clone(), gamma, 1e-5)  # accepted
    fake = type("L", (), {n: staticmethod(no_launch) for n in ("da_gemm_tile_w8", "da_gemm_dk_splitk_w8",
                                                                "da_gemm_resid_rmsnorm_w8")})()
    monkeypatch.setattr(K, "lib", lambda: fake)
    off = torch.zeros(N + 1, dtype=torch.float32, device=DEV)[1:]  # 4 bytes past a 16-B boundary
    off.copy_(s)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    q3, s3, _ = _weights(N, 96)
    q48, s48 = q[:48], s[:48].contiguous()
    q1k, s1k, _ = _weights(1024, Kd)
    ops = {
        "tile": lambda a_, q_, s_, **kw: K.gemm_tile_w8(a_, q_, s_, **kw),
        "dk": lambda a_, q_, s_, **kw: K.gemm_dk_splitk_w8(a_, q_, s_, **kw),
        "norm": lambda a_, q_, s_, **kw: K.gemm_resid_norm_w8(a_, q_, s_, _rand(a_.shape[0], q_.shape[0]),
                                                              _rand(q_.shape[0]), 1e-5, **kw),
    }
    for name, op in ops.items():
        with pytest.raises(ValueError):
            op(a, _rand(N, Kd), s)                                   # bf16 wq
        with pytest.raises(ValueError):
            op(a, q, s.double())                                     # fp64 sw
        with pytest.raises(ValueError):
            op(a.float(), q, s)                                      # fp32 a
        with pytest.raises(ValueError):
            op(a, q, off)                                            # misaligned sw
        with pytest.raises(ValueError):
            op(_rand(129, Kd), q, s)                                 # M = 129
        with pytest.raises(ValueError):
            op(_rand(40, 96), q3, s3)                                # K % 64
        with pytest.raises(ValueError):
            op(a, q, s[:32])                                         # short sw
    for name in ("tile", "dk"):
        with pytest.raises(ValueError):
            ops[name](a, q48, s48, epi=K.EPI_SWIGLU)                 # SwiGLU with N % 32
        with pytest.raises(ValueError):
            ops[name](a, q, s, epi=K.EPI_GELU)
        with pytest.raises(ValueError):
            ops[name](a, q, s, out=_rand(40, 32))                    # out of another shape
    x1k = _rand(40, 1024)
    with pytest.raises(ValueError):                                  # ssq_out too short (2 parts of 64 floats)
        K.gemm_dk_splitk_w8(a, q1k, s1k, epi=K.EPI_RESID, resid=x1k, ssq_out=ssq[:2 * 64 - 1])
    with pytest.raises(ValueError):                                  # row sums need N % 512 == 0 on this route
        K.gemm_dk_splitk_w8(a, q, s, epi=K.EPI_RESID, resid=x, ssq_out=ssq)
    with pytest.raises(ValueError):
        K.gemm_dk_splitk_w8(_rand(65, Kd), q, s)                     # above the route's rows
    with pytest.raises(ValueError):
        K.gemm_dk_splitk_w8(_rand(32, Kd), q, s)                     # gemm_dk_w8's rows
    with pytest.raises(ValueError):
        K.gemm_tile_w8(_rand(32, Kd), q, s)                          # gemm() runs these rows on another kernel
    with pytest.raises(ValueError):
        K.gemm_resid_norm_w8(_rand(32, Kd), q, s, _rand(32, N), gamma, 1e-5)
    # the C entry points refuse before any launch too
    monkeypatch.undo()
    L = K.lib()
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    out = _rand(40, N)
    p = lambda t: K._ptr(t)  # noqa: E731
    INVALID = 1  # hipErrorInvalidValue
    args = lambda wq, sw, M=40, tile=2: (p(a), Kd, wq, sw, p(out), N, None, None, 0, M, N, Kd, 0, tile, 1, p(ws), K._stream())  # noqa: E731
    assert L.da_gemm_tile_w8(*args(None, p(s))) == INVALID and L.da_gemm_tile_w8(*args(p(q), None)) == INVALID
    assert L.da_gemm_tile_w8(*args(p(q), p(off))) == INVALID and L.da_gemm_tile_w8(*args(p(q), p(s), M=129)) == INVALID
    assert L.da_gemm_tile_w8(*args(p(q), p(s), tile=3)) == INVALID and L.da_gemm_tile_w8(*args(p(q), p(s), tile=1)) == INVALID
    assert L.da_gemm_dk_splitk_w8(p(a), Kd, p(q), p(off), p(out), N, None, None, 0, 40, N, Kd, 0, None, 0, Kd, 0.0,
                                  None, p(ws), 2, K._stream()) == INVALID
    assert L.da_gemm_resid_rmsnorm_w8(p(a), Kd, p(q), p(off), p(out), N, None, p(x), N, 40, N, Kd, 2, 2, p(ws),
                                      p(gamma), 1e-5, p(out), N, K._stream()) == INVALID
    assert L.da_gemm_resid_rmsnorm_w8(p(a), Kd, p(q), p(s), p(out), N, None, p(x), N, 40, N, Kd, 3, 2, p(ws),
                                      p(gamma), 1e-5, p(out), N, K._stream()) == INVALID
    torch.cuda.synchronize()
