"""gemm() launches what ops/gemm_plan.py plans: one small product per family, routed automatically
and with the plan's tile / splits passed back, bit for bit; the library no longer resolves tile 0."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from docagents_amd.ops import gemm_plan as P  # noqa: E402
from docagents_amd.ops import kernels as K  # noqa: E402
from docagents_amd.ops import reference as R  # noqa: E402

DEV = "cuda"


def _rand(*shape, scale=1.0):
    return (torch.randn(*shape, device=DEV) * scale).to(torch.bfloat16)


def _close(a, b, atol, rtol=0.02):
    a, b = a.float(), b.float()
    err = (a - b).abs()
    bad = (err > atol + rtol * b.abs()).sum().item()
    assert bad == 0, f"{bad} / {a.numel()} mismatches, max err {err.max().item():.4g}"


def test_cu_count_is_the_devices():
    n = ctypes.c_int(0)
    assert K.lib().da_device_cu_count(torch.cuda.current_device(), ctypes.byref(n)) == 0
    assert K._cus() == K._cus(torch.device(DEV, torch.cuda.current_device())) == n.value > 0


def _m_256_row_tiles():
    """The fewest rows at which an N = 512 product gets 256-row gemm8p tiles on this device."""
    cus = K._cus()
    return next(M for M in range(P.PREFILL_M, 1 << 17) if P.plan(M, 512, 512, cus=cus).tile == P.TILE_8P_256)


# (family, tile, M, K; N = 512), atol as tests/test_kernels_gpu.py uses for that family
CASES = [("gemv", P.TILE_GEMV, 1, 512, 0.03), ("dk", P.TILE_DK, 8, 512, 0.03), ("dk_splitk", P.TILE_DK, 40, 1024, 0.03),
         ("tile", P.TILE_64x128, 130, 512, 0.03), ("tile", P.TILE_128x64_PF4, 100, 512, 0.03),
         ("gemm8p", P.TILE_8P_128, 640, 512, 0.04), ("gemm8p", P.TILE_8P_256, None, 512, 0.04)]


@pytest.mark.parametrize("family,tile,M,Kd,atol", CASES, ids=[f"{c[0]}-t{c[1]}" for c in CASES])
@pytest.mark.parametrize("epi", [K.EPI_NONE, K.EPI_RESID])
def test_auto_and_explicit_route_same_bits(family, tile, M, Kd, atol, epi):
    M = M or _m_256_row_tiles()
    N = 512
    torch.manual_seed(M + Kd + epi)
    p = P.plan(M, N, Kd, epi, cus=K._cus())
    assert (p.family, p.tile) == (family, tile)
    if K._cus() == 256 and tile == P.TILE_8P_256:
        assert M == 16385  # 2 x 129 128-row tiles: the first grid past one wave of 256 CUs
    a, w = _rand(M, Kd), _rand(N, Kd, scale=Kd ** -0.5)
    resid = _rand(M, N) if epi == K.EPI_RESID else None
    auto = K.gemm(a, w, epi=epi, resid=resid)
    explicit = K.gemm(a, w, epi=epi, resid=resid, tile=p.tile, splits=p.splits)
    assert torch.equal(auto, explicit)
    _close(auto, R.gemm(a, w, epi=epi, resid=resid), atol=atol)


def test_library_rejects_tile_0():
    a, w = _rand(130, 512), _rand(512, 512, scale=512 ** -0.5)
    out = torch.full((130, 512), 777.0, device=DEV, dtype=torch.bfloat16)
    rc = K.lib().da_gemm_bf16(K._ptr(a), a.stride(0), K._ptr(w), K._ptr(out), out.stride(0), None, None, 0,
                              130, 512, 512, K.EPI_NONE, 0, 1, None, None, 0.0, K._stream())
    torch.cuda.synchronize()
    assert rc != 0 and bool((out == 777.0).all())


@pytest.mark.parametrize("N", [3072, 4096, 8192])
def test_dk_parts_is_the_librarys(N):
    assert K.dk_parts(N, 16) == K.lib().da_gemm_dk_parts(N)
