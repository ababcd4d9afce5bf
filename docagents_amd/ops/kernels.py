"""ctypes bindings for the gfx950 kernel library (``_da_kernels.so``).

Every wrapper validates shapes / dtypes / contiguity / device on the host BEFORE launching (a
mis-shaped launch of a hand-written kernel can fault the GPU), launches on PyTorch's current HIP
stream, and raises on any launch error. There is deliberately no silent fallback: on a GPU box,
if the library is missing the import fails loudly (``KernelLibraryMissing``). The fp32 PyTorch
oracles for tests live in ``docagents_amd.ops.reference``.
"""
from __future__ import annotations

import contextlib
import ctypes
import math
import os
import threading
from pathlib import Path

import torch

from . import gemm_plan
from .gemm_plan import (DK_MAX_M, DK_SPLITK_ABOVE, dk_fusable, dk_parts, dk_w8_fusable,  # noqa: F401 - re-exported
                        gemv_fusable, gemv_w4_fusable, gemv_w8_fusable, keeps_w4_copy, keeps_w8_copy,
                        prefill_w8_fusable, tile_w8_fusable, weight_op)
from .reference import (dequant_mxfp4, quant_weight_fp8, quant_weight_fp8_pow2,  # noqa: F401 - host-side torch, done
                        quant_weight_mxfp4)                                       # once at load

_LIB = None
_LOCK = threading.Lock()
# DA_KERNELS_DEBUG=1: the -DDA_DEBUG build (device asserts: bounds / shape preconditions inside the
# kernels; python -m docagents_amd.ops.build --debug) instead of the -O3 library
_DEBUG = os.environ.get("DA_KERNELS_DEBUG", "0") == "1"
_LIB_PATH = Path(__file__).resolve().parent / ("_da_kernels_debug.so" if _DEBUG else "_da_kernels.so")

EPI_NONE, EPI_BIAS, EPI_GELU, EPI_SWIGLU, EPI_RESID = 0, 1, 2, 3, 4
EPI_ROPE = 6  # gemm8p only: QKV + RoPE + KV-cache write

c_longlong = ctypes.c_longlong
c_void_p, c_int, c_float, c_uint, c_size_t = (ctypes.c_void_p, ctypes.c_int, ctypes.c_float,
                                             ctypes.c_uint, ctypes.c_size_t)

_SIGS = {
    "da_gemm_bf16": [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int,
                     c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_float, c_void_p],
    "da_gemm_rope": [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int] + [c_void_p] * 5
                    + [c_int] * 5 + [c_void_p],
    "da_gemm_fp8": [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int,
                    c_int, c_int, c_int, c_int, c_void_p],
    "da_gemv_w8": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_float,
                   c_void_p],
    "da_gemv_w4": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_float,
                   c_void_p],
    "da_quant_fp8_rows": [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p],
    "da_layernorm_q": [c_void_p] * 7 + [c_int, c_int, c_float, c_void_p],
    "da_bert_embed_ln_q": [c_void_p] * 11 + [c_int, c_int, c_float, c_void_p],
    "da_gemm_resid_rmsnorm": [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int,
                              c_int, c_int, c_int, c_void_p, c_void_p, c_float, c_void_p, c_int, c_void_p],
    "da_rmsnorm": [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p],
    "da_rmsnorm_routed": [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_int,
                          c_void_p],
    "da_rmsnorm_q8": [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_float, c_int, c_void_p],
    "da_swiglu_interleaved": [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p],
    "da_layernorm": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_void_p],
    "da_bert_embed_ln": [c_void_p] * 9 + [c_int, c_int, c_float, c_void_p],
    "da_embed": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p],
    "da_pool_l2norm": [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p],
    "da_rope_cache": [c_void_p] * 6 + [c_int] * 6 + [c_void_p],
    "da_sample": [c_void_p, c_int, c_int, c_int, c_float, c_uint, c_uint] + [c_void_p] * 9
                 + [c_int] * 5 + [c_void_p],
    "da_flash_attn_v2": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int,
                         c_int, c_int, c_int, c_int, c_float, c_void_p, c_int, c_void_p, c_void_p, c_longlong,
                         c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p],
    "da_malloc_uncached": [c_longlong, ctypes.POINTER(c_void_p)],
    "da_gemm_dk": [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                   c_int, c_void_p, c_int, c_int, c_float, c_void_p, c_void_p],
    "da_gemm_dk_parts": [c_int],
    "da_gemm_dk_w8": [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int,
                      c_int, c_int, c_void_p, c_int, c_int, c_float, c_void_p, c_void_p],
    "da_gemm_dk_splitk": [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                          c_int, c_void_p, c_int, c_int, c_float, c_void_p, c_void_p, c_int, c_void_p],
    "da_gemm_tile_w8": [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int,
                        c_int, c_int, c_int, c_int, c_void_p, c_void_p],
    "da_gemm_dk_splitk_w8": [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int,
                             c_int, c_int, c_int, c_void_p, c_int, c_int, c_float, c_void_p, c_void_p, c_int, c_void_p],
    "da_gemm_resid_rmsnorm_w8": [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int,
                                 c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_float, c_void_p, c_int, c_void_p],
    "da_gemm_tile_w8_nt": [c_int],
    "da_decode_attn": [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                       c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                       c_int, c_void_p],
    "da_rope_cache_kv8": [c_void_p] * 8 + [c_int] * 6 + [c_void_p],
    "da_kv8_dequant": [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p],
    "da_decode_attn_kv8": [c_void_p, c_int] + [c_void_p] * 7 + [c_int] * 7 + [c_float, c_void_p, c_void_p, c_int,
                                                                                c_void_p, c_void_p],
    "da_topk_dense": [c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_float, c_int,
                      c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "da_topk_dense_stream": [c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_float, c_int,
                             c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "da_topk_ranges": [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int,
                       c_float, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "da_topk_merge": [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p],
    "da_index_quant_rows": [c_void_p, c_int, c_int, c_void_p, c_void_p, c_longlong, c_void_p],
    "da_index_quant_scatter": [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_longlong, c_void_p],
    "da_index_dequant_rows": [c_void_p, c_void_p, c_longlong, c_int, c_longlong, c_void_p, c_int, c_void_p, c_void_p],
    "da_kmeans_accum8": [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p],
    "da_topk_dense_stream8": [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_float,
                              c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "da_topk_ranges8": [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int,
                        c_float, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "da_kmeans_accum": [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "da_sample_partial": [c_void_p, c_int, c_int, c_int, c_int, c_float, c_uint, c_uint, c_void_p, c_void_p, c_void_p],
    "da_sample_chunked": [c_void_p, c_int, c_int, c_int, c_float, c_uint, c_uint] + [c_void_p] * 10
                         + [c_int] * 5 + [c_void_p],
    "da_sample_finalize": [c_void_p, c_int, c_int] + [c_void_p] * 8 + [c_int] * 5 + [c_void_p],
    "da_stream_create_cumask": [c_uint, ctypes.POINTER(c_uint), ctypes.POINTER(c_void_p)],
    "da_stream_get_cumask": [c_void_p, c_uint, ctypes.POINTER(c_uint)],
    "da_stream_destroy": [c_void_p],
    "da_device_cu_count": [c_int, ctypes.POINTER(c_int)],
    "da_placement_probe": [c_void_p, c_int, c_longlong, c_void_p],
    "da_spin": [c_int, c_void_p, c_void_p],
    "da_gemm8p_persist": [c_int],
    "da_gemm4w_variant": [c_int],
    "da_gemm_f16": [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                    c_int, c_void_p],
    "da_flash_attn_f16": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int,
                          c_int, c_int, c_float, c_void_p, c_int, c_void_p],
    "da_layernorm_f16": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_void_p],
    "da_bert_embed_ln_f16": [c_void_p] * 9 + [c_int, c_int, c_float, c_void_p],
    "da_pool_l2norm_f16": [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p],
}


class KernelLibraryMissing(RuntimeError):
    pass


class KernelError(RuntimeError):
    pass


def lib() -> ctypes.CDLL:
    """Load (building on first use if sources are newer) the kernel library."""
    global _LIB
    if _LIB is not None:
        return _LIB
    with _LOCK:
        if _LIB is not None:
            return _LIB
        if os.environ.get("DA_BUILD_ON_IMPORT", "1") == "1":
            try:
                from .build import build
                build(debug=_DEBUG)
            except Exception as e:  # noqa: BLE001 - fall through to the explicit check below
                if not _LIB_PATH.exists():
                    raise KernelLibraryMissing(f"cannot build {_LIB_PATH}: {e}") from e
        if not _LIB_PATH.exists():
            raise KernelLibraryMissing(f"{_LIB_PATH} not built; run python -m docagents_amd.ops.build")
        import torch.cuda  # noqa: F401 - make sure torch's HIP runtime is loaded first
        L = ctypes.CDLL(str(_LIB_PATH))
        for name, argt in _SIGS.items():
            fn = getattr(L, name)
            fn.argtypes = argt
            fn.restype = c_int
        L.da_topk_dense_ws.argtypes = [c_int, c_int, c_int, c_int]
        L.da_topk_dense_ws.restype = c_size_t
        L.da_topk_stream_ws.argtypes = [c_int, c_int, c_int, c_int]
        L.da_topk_stream_ws.restype = c_size_t
        L.da_topk_dense_stream8_ws.argtypes = [c_int, c_int, c_int, c_int]
        L.da_topk_dense_stream8_ws.restype = c_size_t
        _LIB = L
        return L


def available() -> bool:
    return torch.cuda.is_available() and _LIB_PATH.exists()


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(rc: int, name: str):
    if rc != 0:
        raise KernelError(f"{name} failed with hipError {rc}")


def _req(cond: bool, msg: str):
    if not cond:
        raise ValueError(msg)


def _bf16_cuda(t, name):
    _req(t.is_cuda, f"{name} must be on GPU")
    _req(t.dtype == torch.bfloat16, f"{name} must be bf16, got {t.dtype}")


def _i32(t, name):
    _req(t.is_cuda and t.dtype == torch.int32 and t.is_contiguous(), f"{name} must be contiguous int32 on GPU")


MAX_ROW_D = 16384  # norm.hip: 8 chunks of 8 elements per thread, 256 threads


def _row_d(D: int, name: str):
    _req(D % 8 == 0 and 0 < D <= MAX_ROW_D, f"{name}: D = {D} must be a multiple of 8, at most {MAX_ROW_D}")


def _row_vec(t, D: int, dtype, name: str):
    """A [D] operand the launcher reads as D contiguous elements of dtype."""
    _req(t.is_cuda and t.dtype == dtype and t.numel() == D and t.is_contiguous(), f"{name} must be contiguous {dtype} [D]")


def _row_table(t, D: int, dtype, name: str):
    _req(t.is_cuda and t.dtype == dtype and t.dim() == 2 and t.shape[1] == D and t.is_contiguous(),
         f"{name} must be contiguous {dtype} [rows, D]")


def _row_out(t, rows: int, D: int, dtype, name: str):
    """An output the launcher writes as `rows` contiguous rows of D elements of dtype."""
    _req(t.is_cuda and t.dtype == dtype and t.dim() == 2 and t.shape[1] == D and t.shape[0] >= rows
         and t.is_contiguous(), f"{name} must be contiguous {dtype} [>= {rows}, {D}]")


def _pool_outs(B: int, D: int, out32, out16):
    if out32 is not None:
        _row_out(out32, B, D, torch.float32, "out32")
    if out16 is not None:
        _row_out(out16, B, D, torch.bfloat16, "out16")


# ----------------------------------------------------------------------------------- GEMM
_WS = {}
_ROLE = threading.local()


@contextlib.contextmanager
def workspace_role(name: str):
    """Kernels launched inside this context use the split-K / decode workspace of ``name``
    instead of the default one. Two phases that run CONCURRENTLY on different streams (the
    serving pipeline's prefill lane next to a replaying decode graph) must not share scratch:
    the decode graph captured the default workspace's pointer."""
    prev = getattr(_ROLE, "name", "main")
    _ROLE.name = name
    try:
        yield
    finally:
        _ROLE.name = prev


def workspace_buffer(device):
    """The current role's workspace tensor on ``device`` (None before its first use): callers that
    capture graphs check it is the same object after their captures (a grown workspace frees the
    buffer earlier captures point at)."""
    device = torch.device(device)
    key = (device.index if device.index is not None else torch.cuda.current_device(), getattr(_ROLE, "name", "main"))
    return _WS.get(key)


def _workspace(nbytes: int, device) -> torch.Tensor:
    key = (device.index if device.index is not None else torch.cuda.current_device(), getattr(_ROLE, "name", "main"))
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _WS[key] = buf
    return buf


_CUS = {}


def _cus(device=None) -> int:
    """CU count of ``device`` (default: the current one), read once per device: gemm_plan's input."""
    idx = torch.cuda.current_device() if device is None or device.index is None else device.index
    n = _CUS.get(idx)
    if n is None:
        n = _CUS[idx] = torch.cuda.get_device_properties(idx).multi_processor_count
    return n


def gemm(a: torch.Tensor, w: torch.Tensor, bias=None, epi: int = EPI_NONE, resid=None, out=None,
         tile: int = 0, splits: int = 0, rms=None) -> torch.Tensor:
    """out[M, N'] = epi(a[M, K] @ w[N, K]^T). N' = N/2 for EPI_SWIGLU (w rows interleaved by 16).
    rms = (gamma, eps): ``a`` is the raw residual stream and RMSNorm(a) * gamma is fused into the
    GEMV (M == 1 only, see gemv_fusable); gamma None = unit gain (folded into ``w``)."""
    _bf16_cuda(a, "a"); _bf16_cuda(w, "w")
    _req(a.dim() == 2 and w.dim() == 2, "gemm expects 2-D operands")
    M, K = a.shape
    N, K2 = w.shape
    _req(K == K2, f"K mismatch {K} vs {K2}")
    p = gemm_plan.plan(M, N, K, epi, cus=_cus(a.device), tile=tile, splits=splits, rms=rms is not None)
    _req(a.stride(1) == 1 and a.stride(0) % 8 == 0 and a.stride(0) >= K, "a must be row-major, 16-B aligned rows")
    _req(w.is_contiguous(), "w must be contiguous")
    _req(a.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0, "operands must be 16-B aligned")
    nout = N // 2 if epi == EPI_SWIGLU else N
    if out is None:
        out = torch.empty((M, nout), dtype=torch.bfloat16, device=a.device)
    _bf16_cuda(out, "out")
    _req(out.shape == (M, nout) and out.stride(1) == 1 and out.stride(0) % 8 == 0, "bad out")
    if bias is not None:
        _bf16_cuda(bias, "bias"); _req(bias.numel() == N and bias.is_contiguous(), "bias must be [N]")
        _req(epi in (EPI_BIAS, EPI_GELU, EPI_RESID), "bias only with BIAS/GELU/RESID epilogues")
    ldr = 0
    if epi == EPI_RESID:
        _req(resid is not None, "EPI_RESID needs resid")
        _bf16_cuda(resid, "resid")
        _req(resid.shape == (M, N) and resid.stride(1) == 1 and resid.stride(0) % 8 == 0, "bad resid")
        ldr = resid.stride(0)
    if M == 0:
        return out
    if p.family in ("dk", "dk_splitk"):
        return gemm_dk(a, w, epi=epi, bias=bias, resid=resid, out=out)
    gamma, eps = (None, 0.0) if rms is None else rms  # rms = (gain or None for unit gain, eps > 0)
    if rms is not None:
        _req(eps > 0, "fused RMSNorm needs eps > 0")
        if gamma is not None:
            _bf16_cuda(gamma, "gamma"); _req(gamma.numel() == K, "gamma must be [K]")
    ws = _workspace(p.ws_bytes, a.device) if p.ws_bytes else None
    rc = lib().da_gemm_bf16(_ptr(a), a.stride(0), _ptr(w), _ptr(out), out.stride(0), _ptr(bias), _ptr(resid), ldr,
                            M, N, K, epi, p.tile, p.splits, _ptr(ws), _ptr(gamma), float(eps), _stream())
    _check(rc, "gemm")
    return out


def gemm_route(M: int, N: int, K: int, epi: int = EPI_NONE):
    """The prefill routing of gemm() at M rows, as keywords for gemm(): {"tile": t, "splits": s}.
    A product over a subset of those rows run with them (gemm(a[idx], w, **gemm_route(M, N, K, epi)))
    goes through the same tile kernel with the same K order and split count as the full launch, so
    each row gets the bits the full launch gives it (GEMM rows are independent; the persistent and
    the one-tile-per-workgroup forms of gemm8p are bit-identical). None for M <= 128: those go to
    the GEMV / gemm_dk / weight-streaming family, chosen by more than the tile number."""
    if M <= 128:
        return None
    p = gemm_plan.plan(M, N, K, epi, cus=_cus())
    return {"tile": p.tile, "splits": p.splits}


def _dk_operands(name, a, N, max_m, epi, bias, resid, out, norm_in, ssq_out):
    """The operand checks gemm_dk and gemm_dk_w8 share (everything but the weights; every pointer the
    kernel body reads or writes 16 B at a time is 16-B aligned). Allocates ``out`` if None. Returns
    (M, N, K, nout, out, ldr, ssq, parts, eps); raises ValueError before any launch."""
    _bf16_cuda(a, "a")
    _req(a.dim() == 2, f"{name} expects 2-D operands")
    M, K = a.shape
    _req(1 <= M <= max_m and K >= 256 and K % 256 == 0 and N >= 16 and N % 16 == 0, f"{name} shape M={M} N={N} K={K}")
    _req(epi in (EPI_NONE, EPI_BIAS, EPI_RESID, EPI_SWIGLU) and (epi != EPI_SWIGLU or N % 32 == 0),
         f"{name} does not take epi={epi} at N={N}")
    _req(a.stride(1) == 1 and a.stride(0) % 8 == 0 and a.stride(0) >= K and a.data_ptr() % 16 == 0,
         "a must be row-major, 16-B aligned rows")
    nout = N // 2 if epi == EPI_SWIGLU else N
    if out is None:
        out = torch.empty((M, nout), dtype=torch.bfloat16, device=a.device)
    _bf16_cuda(out, "out")
    _req(out.shape == (M, nout) and out.stride(1) == 1 and out.stride(0) % 8 == 0 and out.data_ptr() % 16 == 0,
         "bad out")
    if bias is not None:
        _bf16_cuda(bias, "bias")
        _req(bias.numel() == N and bias.is_contiguous() and bias.data_ptr() % 16 == 0, "bias must be [N]")
        _req(epi in (EPI_BIAS, EPI_RESID), "bias only with BIAS/RESID epilogues")
    ldr = 0
    if epi == EPI_RESID:
        _req(resid is not None, "EPI_RESID needs resid")
        _bf16_cuda(resid, "resid")
        _req(resid.shape == (M, N) and resid.stride(1) == 1 and resid.stride(0) % 8 == 0
             and resid.data_ptr() % 16 == 0, "bad resid")
        ldr = resid.stride(0)
    ssq, parts, eps = (None, 0, 0.0) if norm_in is None else norm_in
    if ssq is not None:
        _req(epi != EPI_RESID, "a residual producer takes no deferred norm")
        _req(ssq.is_cuda and ssq.dtype == torch.float32 and ssq.is_contiguous() and parts >= 1
             and ssq.numel() >= parts * 64 and ssq.data_ptr() % 16 == 0 and eps > 0, "bad ssq_in")
    if ssq_out is not None:
        _req(epi == EPI_RESID, "ssq_out needs the residual epilogue")
        _req(ssq_out.is_cuda and ssq_out.dtype == torch.float32 and ssq_out.is_contiguous()
             and ssq_out.numel() >= dk_parts(N, M) * 64, "bad ssq_out")
    return M, N, K, nout, out, ldr, ssq, parts, eps


def gemm_dk(a, w, epi: int = EPI_NONE, bias=None, resid=None, out=None, norm_in=None, ssq_out=None):
    """Decode-sized product (1 <= M <= 64) in one launch without split-K:
    out = epi(rownorm(a) @ w^T). norm_in = (ssq, parts, eps): ``a`` is the raw residual stream and
    each row is scaled by rsqrt(sum of ssq[:parts, row] / K + eps) first (bf16-rounded, as the
    rmsnorm kernel would; RMSNorm gains folded into w). ssq_out (EPI_RESID only): fp32
    [dk_parts(N), 64] receives the per-part sums of squares of the new rows, for the next consumer."""
    _bf16_cuda(w, "w")
    _req(w.dim() == 2 and w.is_contiguous() and w.data_ptr() % 16 == 0, "w must be contiguous, 16-B aligned")
    M, N, K, _, out, ldr, ssq, parts, eps = _dk_operands("gemm_dk", a, w.shape[0], DK_MAX_M, epi, bias, resid, out,
                                                         norm_in, ssq_out)
    _req(w.shape[1] == K, f"K mismatch {K} vs {w.shape[1]}")
    if epi != EPI_RESID:
        resid = None
    p = gemm_plan.plan_dk(M, N, K, ssq_out is not None)
    if p.family == "dk_splitk":
        ws = _workspace(p.ws_bytes, a.device)
        _check(lib().da_gemm_dk_splitk(_ptr(a), a.stride(0), _ptr(w), _ptr(out), out.stride(0), _ptr(bias), _ptr(resid),
                                       ldr, M, N, K, epi, _ptr(ssq), parts, K, float(eps), _ptr(ssq_out), _ptr(ws),
                                       p.splits, _stream()), "gemm_dk_splitk")
        return out
    _check(lib().da_gemm_dk(_ptr(a), a.stride(0), _ptr(w), _ptr(out), out.stride(0), _ptr(bias), _ptr(resid), ldr,
                            M, N, K, epi, _ptr(ssq), parts, K, float(eps), _ptr(ssq_out), _stream()), "gemm_dk")
    return out


# Every GEMM runs on the in-tree kernels: gemm8p (phase-split BMx256, csrc/gemm8p.hip) from 256
# rows, the 64x128 / 32x128 weight-streaming tiles + split-K below, the GEMV at batch 1. The
# vendor-library arms used for comparisons live in bench/ab_arms.py (same-box measurements:
# profiles/r2/ab_gemm8p_vs_hipblaslt.txt).


def gemm_rope(a, w, pos, cos_sin, H: int, Hkv: int, D: int, slot, k_cache, v_cache, out=None,
              kv_out: bool = True) -> torch.Tensor:
    """Prefill QKV projection: qkv = a @ w^T with RoPE applied to the q / k heads and the token's
    k / v written to the KV cache (cache [slots, Hkv, max_seq, D]) — one kernel (gemm8p EPI_ROPE)
    from 256 rows; shorter prefills run gemm + rope_cache (identical roundings). kv_out=False: the
    k / v columns of the result may be left unwritten (the attention reads the cache; see
    flash_attn_varlen kv_cache) — only the q columns are defined."""
    _bf16_cuda(a, "a"); _bf16_cuda(w, "w"); _i32(pos, "pos"); _i32(slot, "slot")
    M, K = a.shape
    N = w.shape[0]
    _req(N == (H + 2 * Hkv) * D and w.shape[1] == K and D % 8 == 0, "qkv weight shape")
    _req(pos.numel() >= M and slot.numel() >= M, "pos / slot length")
    _req(cos_sin.dtype == torch.float32 and cos_sin.is_contiguous() and cos_sin.shape[1] == D // 2, "cos_sin")
    _req(k_cache.is_contiguous() and v_cache.is_contiguous() and k_cache.shape == v_cache.shape
         and k_cache.dim() == 4 and k_cache.shape[1] == Hkv and k_cache.shape[3] == D, "caches")
    if M < 256 or K % 64 or K < 128 or a.stride(1) != 1 or a.stride(0) % 8 or not w.is_contiguous():
        qkv = gemm(a, w, out=out)
        return rope_cache(qkv, pos, cos_sin, H, Hkv, D, slot=slot, k_cache=k_cache, v_cache=v_cache)
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=a.device)
    _req(out.shape == (M, N) and out.stride(1) == 1 and out.stride(0) % 8 == 0, "bad out")
    _check(lib().da_gemm_rope(_ptr(a), a.stride(0), _ptr(w), _ptr(out), out.stride(0), M, N, K, _ptr(pos), _ptr(slot),
                              _ptr(cos_sin), _ptr(k_cache), _ptr(v_cache), H, Hkv, D, k_cache.shape[2], int(kv_out),
                              _stream()),
           "gemm_rope")
    return out


FP8 = torch.float8_e4m3fn  # OCP e4m3 (gfx950), not the MI300 fnuz variant


def quant_fp8(x: torch.Tensor, out=None, scale=None):
    """Per-row dynamic e4m3 quantisation: returns (q [M, K] float8_e4m3fn, scale [M] fp32)."""
    _bf16_cuda(x, "x")
    _req(x.dim() == 2 and x.stride(1) == 1 and x.stride(0) % 8 == 0 and x.shape[1] % 8 == 0, "x layout")
    M, K = x.shape
    _row_d(K, "quant_fp8")
    if out is None:
        out = torch.empty((M, K), dtype=FP8, device=x.device)
    if scale is None:
        scale = torch.empty(M, dtype=torch.float32, device=x.device)
    _req(out.dtype == FP8 and out.shape == (M, K) and out.stride(1) == 1 and out.stride(0) % 16 == 0, "bad out")
    _req(scale.dtype == torch.float32 and scale.numel() >= M, "bad scale")
    _check(lib().da_quant_fp8_rows(_ptr(x), x.stride(0), M, K, _ptr(out), out.stride(0), _ptr(scale), _stream()),
           "quant_fp8")
    return out, scale


def gemm_w8(a: torch.Tensor, wq: torch.Tensor, sw: torch.Tensor, bias=None, epi: int = EPI_NONE, resid=None,
            out=None, rms=None) -> torch.Tensor:
    """out[1, N'] = epi((a[1, K] @ wq[N, K]^T) * sw[None, :]) with e4m3 weights and fp32 row scales
    (N' = N/2 for EPI_SWIGLU). rms = (gamma or None, eps): RMSNorm(a) fused, as in gemm()."""
    _bf16_cuda(a, "a")
    _req(wq.is_cuda and wq.dtype == FP8, f"wq must be float8_e4m3fn on GPU, got {wq.dtype}")
    _req(a.dim() == 2 and wq.dim() == 2, "gemm_w8 expects 2-D operands")
    M, K = a.shape
    N, K2 = wq.shape
    _req(K == K2, f"K mismatch {K} vs {K2}")
    _req(gemv_w8_fusable(M, N, K, epi), f"gemm_w8 does not take M={M} N={N} K={K} epi={epi}")
    _req(a.stride(1) == 1, "a must be a contiguous row")
    _req(wq.is_contiguous(), "wq must be contiguous")
    _req(a.data_ptr() % 16 == 0 and wq.data_ptr() % 16 == 0, "operands must be 16-B aligned")
    _req(sw.is_cuda and sw.dtype == torch.float32 and sw.is_contiguous() and sw.shape == (N,), "sw must be fp32 [N]")
    nout = N // 2 if epi == EPI_SWIGLU else N
    if out is None:
        out = torch.empty((M, nout), dtype=torch.bfloat16, device=a.device)
    _bf16_cuda(out, "out")
    _req(out.shape == (M, nout) and out.stride(1) == 1, "bad out")
    if bias is not None:
        _bf16_cuda(bias, "bias"); _req(bias.numel() == N and bias.is_contiguous(), "bias must be [N]")
        _req(epi in (EPI_BIAS, EPI_RESID), "bias only with BIAS/RESID epilogues")
    if epi == EPI_RESID:
        _req(resid is not None, "EPI_RESID needs resid")
        _bf16_cuda(resid, "resid")
        _req(resid.shape == (M, N) and resid.stride(1) == 1, "bad resid")
    else:
        resid = None
    gamma, eps = (None, 0.0) if rms is None else rms
    if rms is not None:
        _req(eps > 0, "fused RMSNorm needs eps > 0")
        if gamma is not None:
            _bf16_cuda(gamma, "gamma")
            _req(gamma.numel() == K and gamma.is_contiguous() and gamma.data_ptr() % 16 == 0, "gamma must be [K]")
    if N == 0:
        return out
    _check(lib().da_gemv_w8(_ptr(a), _ptr(wq), _ptr(sw), _ptr(out), _ptr(bias), _ptr(resid), N, K, epi, _ptr(gamma),
                            float(eps), _stream()), "gemm_w8")
    return out


def gemm_w4(a: torch.Tensor, wq: torch.Tensor, se: torch.Tensor, bias=None, epi: int = EPI_NONE, resid=None,
            out=None, rms=None) -> torch.Tensor:
    """out[1, N'] = epi(a[1, K] @ dq(wq, se)[N, K]^T) with MXFP4 weights: e2m1 codes wq uint8 [N, K/2] and
    e8m0 scale bytes se uint8 [N, K/32] (reference.quant_weight_mxfp4's layout; N' = N/2 for EPI_SWIGLU).
    rms = (gamma or None, eps): RMSNorm(a) fused, as in gemm(). Anything the kernel would refuse raises
    ValueError before any launch."""
    _bf16_cuda(a, "a")
    _req(wq.is_cuda and wq.dtype == torch.uint8, f"wq must be uint8 (e2m1 codes) on GPU, got {wq.dtype}")
    _req(se.is_cuda and se.dtype == torch.uint8, f"se must be uint8 (e8m0 scales) on GPU, got {se.dtype}")
    _req(a.dim() == 2 and wq.dim() == 2 and se.dim() == 2, "gemm_w4 expects 2-D operands")
    M, K = a.shape
    N = wq.shape[0]
    _req(wq.shape[1] * 2 == K, f"K mismatch {K} vs {wq.shape[1] * 2} (two codes per byte)")
    _req(gemv_w4_fusable(M, N, K, epi), f"gemm_w4 does not take M={M} N={N} K={K} epi={epi}")
    _req(se.shape == (N, K // 32), f"se must be [N, K/32] = {(N, K // 32)}, got {tuple(se.shape)}")
    _req(a.stride(1) == 1, "a must be a contiguous row")
    _req(wq.is_contiguous() and se.is_contiguous(), "wq and se must be contiguous")
    _req(a.data_ptr() % 16 == 0 and wq.data_ptr() % 16 == 0 and se.data_ptr() % 16 == 0,
         "operands must be 16-B aligned")
    nout = N // 2 if epi == EPI_SWIGLU else N
    if out is None:
        out = torch.empty((M, nout), dtype=torch.bfloat16, device=a.device)
    _bf16_cuda(out, "out")
    _req(out.shape == (M, nout) and out.stride(1) == 1, "bad out")
    if bias is not None:
        _bf16_cuda(bias, "bias"); _req(bias.numel() == N and bias.is_contiguous(), "bias must be [N]")
        _req(epi in (EPI_BIAS, EPI_RESID), "bias only with BIAS/RESID epilogues")
    if epi == EPI_RESID:
        _req(resid is not None, "EPI_RESID needs resid")
        _bf16_cuda(resid, "resid")
        _req(resid.shape == (M, N) and resid.stride(1) == 1, "bad resid")
    else:
        resid = None
    gamma, eps = (None, 0.0) if rms is None else rms
    if rms is not None:
        _req(eps > 0, "fused RMSNorm needs eps > 0")
        if gamma is not None:
            _bf16_cuda(gamma, "gamma")
            _req(gamma.numel() == K and gamma.is_contiguous() and gamma.data_ptr() % 16 == 0, "gamma must be [K]")
    if N == 0:
        return out
    _check(lib().da_gemv_w4(_ptr(a), _ptr(wq), _ptr(se), _ptr(out), _ptr(bias), _ptr(resid), N, K, epi, _ptr(gamma),
                            float(eps), _stream()), "gemm_w4")
    return out


def gemm_dk_w8(a, wq, sw, epi: int = EPI_NONE, bias=None, resid=None, out=None, norm_in=None, ssq_out=None):
    """gemm_dk on e4m3 weights with fp32 row scales (1 <= M <= 32), one launch:
    out = epi((rownorm(a) @ wq^T) * sw[None, :]). norm_in / ssq_out as gemm_dk (dk_parts(N, M) parts: a residual
    producer tiles like gemm_dk's). Anything the kernel would refuse raises ValueError before any launch."""
    _req(wq.is_cuda and wq.dtype == FP8, f"wq must be float8_e4m3fn on GPU, got {wq.dtype}")
    _req(wq.dim() == 2 and wq.is_contiguous() and wq.data_ptr() % 16 == 0, "wq must be contiguous, 16-B aligned")
    M, N, K, _, out, ldr, ssq, parts, eps = _dk_operands("gemm_dk_w8", a, wq.shape[0], gemm_plan.DK_W8_MAX_M, epi,
                                                         bias, resid, out, norm_in, ssq_out)
    _req(wq.shape[1] == K, f"K mismatch {K} vs {wq.shape[1]}")
    _req(sw.is_cuda and sw.dtype == torch.float32 and sw.is_contiguous() and sw.shape == (N,)
         and sw.data_ptr() % 16 == 0, "sw must be fp32 [N], 16-B aligned")
    if epi != EPI_RESID:
        resid = None
    _check(lib().da_gemm_dk_w8(_ptr(a), a.stride(0), _ptr(wq), _ptr(sw), _ptr(out), out.stride(0), _ptr(bias),
                               _ptr(resid), ldr, M, N, K, epi, _ptr(ssq), parts, K, float(eps), _ptr(ssq_out),
                               _stream()), "gemm_dk_w8")
    return out


def _w8_weights(name, wq, sw, K):
    """The e4m3 weight copy of the 33..128-row ops: codes [N, K] and fp32 row scales [N], both read 16 B
    at a time. Returns N."""
    _req(wq.is_cuda and wq.dtype == FP8, f"wq must be float8_e4m3fn on GPU, got {wq.dtype}")
    _req(wq.dim() == 2 and wq.is_contiguous() and wq.data_ptr() % 16 == 0, "wq must be contiguous, 16-B aligned")
    _req(wq.shape[1] == K, f"{name}: K mismatch {K} vs {wq.shape[1]}")
    N = wq.shape[0]
    _req(sw.is_cuda and sw.dtype == torch.float32 and sw.is_contiguous() and sw.shape == (N,)
         and sw.data_ptr() % 16 == 0, "sw must be fp32 [N], 16-B aligned")
    return N


def _tile_operands(name, a, N, epi, bias, resid, out):
    """The operand checks of gemm_tile_w8 (gemm()'s, with every pointer 16-B aligned and the rows the
    fp8 tiles take). Allocates ``out`` if None. Returns (M, K, out, ldr)."""
    _bf16_cuda(a, "a")
    _req(a.dim() == 2, f"{name} expects 2-D operands")
    M, K = a.shape
    _req(1 <= M <= gemm_plan.TILE_W8_MAX_M and K >= 64 and K % 64 == 0 and N >= 8 and N % 8 == 0,
         f"{name} shape M={M} N={N} K={K}")
    _req(epi in (EPI_NONE, EPI_BIAS, EPI_RESID, EPI_SWIGLU) and (epi != EPI_SWIGLU or N % 32 == 0),
         f"{name} does not take epi={epi} at N={N}")
    _req(a.stride(1) == 1 and a.stride(0) % 8 == 0 and a.stride(0) >= K and a.data_ptr() % 16 == 0,
         "a must be row-major, 16-B aligned rows")
    nout = N // 2 if epi == EPI_SWIGLU else N
    if out is None:
        out = torch.empty((M, nout), dtype=torch.bfloat16, device=a.device)
    _bf16_cuda(out, "out")
    _req(out.shape == (M, nout) and out.stride(1) == 1 and out.stride(0) % 8 == 0 and out.stride(0) >= nout
         and out.data_ptr() % 16 == 0, "bad out")
    if bias is not None:
        _bf16_cuda(bias, "bias")
        _req(bias.numel() == N and bias.is_contiguous() and bias.data_ptr() % 16 == 0, "bias must be [N]")
        _req(epi in (EPI_BIAS, EPI_RESID), "bias only with BIAS/RESID epilogues")
    ldr = 0
    if epi == EPI_RESID:
        _req(resid is not None, "EPI_RESID needs resid")
        _bf16_cuda(resid, "resid")
        _req(resid.shape == (M, N) and resid.stride(1) == 1 and resid.stride(0) % 8 == 0 and resid.stride(0) >= N
             and resid.data_ptr() % 16 == 0, "bad resid")
        ldr = resid.stride(0)
    return M, K, out, ldr


def gemm_tile_w8(a, wq, sw, epi: int = EPI_NONE, bias=None, resid=None, out=None) -> torch.Tensor:
    """gemm() at 1..128 rows on e4m3 weights with fp32 row scales, on the 64x128 / 128x64 weight-streaming
    tiles: out = epi((a @ wq^T) * sw[None, :]), with the tile, split count and workspace gemm() takes
    for the same product (gemm_plan.plan_tile_w8), so with power-of-two scales the result is gemm()'s
    on the dequantised matrix bit for bit. Anything the kernel would refuse raises ValueError before
    any launch (a product gemm() runs on another tile, e.g. at 32 rows or fewer, included)."""
    _req(a.dim() == 2, "gemm_tile_w8 expects 2-D operands")
    N = _w8_weights("gemm_tile_w8", wq, sw, a.shape[1])
    M, K, out, ldr = _tile_operands("gemm_tile_w8", a, N, epi, bias, resid, out)
    if epi != EPI_RESID:
        resid = None
    p = gemm_plan.plan_tile_w8(M, N, K, epi, cus=_cus(a.device))
    ws = _workspace(p.ws_bytes, a.device) if p.ws_bytes else None
    _check(lib().da_gemm_tile_w8(_ptr(a), a.stride(0), _ptr(wq), _ptr(sw), _ptr(out), out.stride(0), _ptr(bias),
                                 _ptr(resid), ldr, M, N, K, epi, p.tile, p.splits, _ptr(ws), _stream()), "gemm_tile_w8")
    return out


def gemm_dk_splitk_w8(a, wq, sw, epi: int = EPI_NONE, bias=None, resid=None, out=None, norm_in=None, ssq_out=None):
    """gemm_dk's 33..64-row split-K route on e4m3 weights with fp32 row scales:
    out = epi((rownorm(a) @ wq^T) * sw[None, :]), norm_in / ssq_out as gemm_dk (an ssq_out needs
    N % 512 == 0: one part per 512 columns, dk_parts(N, M)). The split count and workspace are
    plan_dk's. Anything the kernel would refuse raises ValueError before any launch."""
    _req(a.dim() == 2, "gemm_dk_splitk_w8 expects 2-D operands")
    N = _w8_weights("gemm_dk_splitk_w8", wq, sw, a.shape[1])
    _req(DK_SPLITK_ABOVE < a.shape[0], f"gemm_dk_splitk_w8 takes {DK_SPLITK_ABOVE + 1}..{DK_MAX_M} rows, got {a.shape[0]}")
    M, N, K, _, out, ldr, ssq, parts, eps = _dk_operands("gemm_dk_splitk_w8", a, N, DK_MAX_M, epi, bias, resid, out,
                                                         norm_in, ssq_out)
    _req(out.stride(0) >= out.shape[1] and (ldr == 0 or ldr >= N), "rows of out / resid overlap")
    if epi != EPI_RESID:
        resid = None
    p = gemm_plan.plan_dk_splitk_w8(M, N, K, ssq_out is not None)
    ws = _workspace(p.ws_bytes, a.device)
    _check(lib().da_gemm_dk_splitk_w8(_ptr(a), a.stride(0), _ptr(wq), _ptr(sw), _ptr(out), out.stride(0), _ptr(bias),
                                      _ptr(resid), ldr, M, N, K, epi, _ptr(ssq), parts, K, float(eps), _ptr(ssq_out),
                                      _ptr(ws), p.splits, _stream()), "gemm_dk_splitk_w8")
    return out


def gemm_resid_norm_w8(a, wq, sw, resid, gamma, eps: float, out=None, h_out=None, bias=None):
    """gemm_resid_norm at 33..128 rows on e4m3 weights with fp32 row scales: out = resid +
    (a @ wq^T) * sw[None, :] (+ bias) and h_out = RMSNorm(out) * gamma, on plan_resid_norm's tile and
    split count. Returns h_out. Anything the kernel would refuse raises ValueError before any launch."""
    _bf16_cuda(a, "a"); _bf16_cuda(resid, "resid"); _bf16_cuda(gamma, "gamma")
    _req(a.dim() == 2, "gemm_resid_norm_w8 expects 2-D operands")
    M, K = a.shape
    N = _w8_weights("gemm_resid_norm_w8", wq, sw, K)
    _req(1 <= M <= gemm_plan.TILE_W8_MAX_M and K >= 64 and K % 64 == 0 and N >= 8 and N % 8 == 0 and N <= 8192,
         f"gemm_resid_norm_w8 shape M={M} N={N} K={K}")
    _req(a.stride(1) == 1 and a.stride(0) % 8 == 0 and a.stride(0) >= K and a.data_ptr() % 16 == 0,
         "a must be row-major, 16-B aligned rows")
    _req(gamma.numel() == N and gamma.is_contiguous() and gamma.data_ptr() % 16 == 0 and eps > 0, "gamma must be [N], eps > 0")
    out = resid if out is None else out
    if h_out is None:
        h_out = torch.empty((M, N), dtype=torch.bfloat16, device=a.device)
    for t, nm in ((resid, "resid"), (out, "out"), (h_out, "h_out")):
        _bf16_cuda(t, nm)
        _req(t.shape == (M, N) and t.stride(1) == 1 and t.stride(0) % 8 == 0 and t.stride(0) >= N
             and t.data_ptr() % 16 == 0, f"bad {nm}")
    if bias is not None:
        _bf16_cuda(bias, "bias")
        _req(bias.numel() == N and bias.is_contiguous(), "bias must be [N]")
    p = gemm_plan.plan_resid_norm_w8(M, N, K)
    ws = _workspace(p.ws_bytes, a.device)
    _check(lib().da_gemm_resid_rmsnorm_w8(_ptr(a), a.stride(0), _ptr(wq), _ptr(sw), _ptr(out), out.stride(0),
                                          _ptr(bias), _ptr(resid), resid.stride(0), M, N, K, p.tile, p.splits, _ptr(ws),
                                          _ptr(gamma), float(eps), _ptr(h_out), h_out.stride(0), _stream()),
           "gemm_resid_norm_w8")
    return h_out


def gemm_tile_w8_nt(v: int = -1) -> int:
    """The fp8 tiles' non-temporal code loads: 0 / 1 = every tile without / with, -1 = the per-tile
    rule (csrc/gemm_tile_w8.hip); returns the setting. For A/B runs (bench/w8_mid.py)."""
    return int(lib().da_gemm_tile_w8_nt(int(v)))


def gemm_fp8(aq, sa, wq, sw, bias=None, epi: int = EPI_NONE, resid=None, out=None) -> torch.Tensor:
    """out[M, N'] = epi((aq . wq^T) * sa[:, None] * sw[None, :]) with e4m3 operands (256x256 MFMA tile; N' = N/2
    for EPI_SWIGLU on 16-row gate / up interleaved weights). Any M; rows may be padded (aq, out, resid strides).
    EPI_RESID may add in place (``out is resid``): every element is read and written by the same lane."""
    _req(aq.is_cuda and wq.is_cuda and aq.dtype == FP8 and wq.dtype == FP8, "fp8 operands expected")
    _req(aq.dim() == 2 and wq.dim() == 2, "gemm_fp8 expects 2-D operands")
    M, K = aq.shape
    N, K2 = wq.shape
    _req(K == K2 and K % 128 == 0 and N % 8 == 0, f"fp8 gemm shape M={M} N={N} K={K}")
    _req(epi in (EPI_NONE, EPI_BIAS, EPI_GELU, EPI_SWIGLU, EPI_RESID), f"gemm_fp8 has no epilogue {epi}")
    _req(epi != EPI_SWIGLU or N % 32 == 0, f"fp8 gemm SwiGLU needs N % 32 == 0, got N={N}")
    _req(aq.stride(1) == 1 and aq.stride(0) % 16 == 0 and aq.stride(0) >= K and wq.is_contiguous(),
         "fp8 operand layout")
    _req(aq.data_ptr() % 16 == 0 and wq.data_ptr() % 16 == 0, "operands must be 16-B aligned")
    _req(sa.is_cuda and sw.is_cuda and sa.dtype == torch.float32 and sa.is_contiguous() and sa.numel() >= M
         and sw.dtype == torch.float32 and sw.is_contiguous() and sw.numel() == N, "scales")
    nout = N // 2 if epi == EPI_SWIGLU else N
    if out is None:
        out = torch.empty((M, nout), dtype=torch.bfloat16, device=aq.device)
    _bf16_cuda(out, "out")
    _req(out.shape == (M, nout) and out.stride(1) == 1 and out.stride(0) % 8 == 0 and out.stride(0) >= nout
         and out.data_ptr() % 16 == 0, "bad out")
    if bias is not None:
        _bf16_cuda(bias, "bias"); _req(bias.numel() == N and bias.is_contiguous(), "bias must be [N]")
    ldr = 0
    if epi == EPI_RESID:
        _req(resid is not None, "EPI_RESID needs resid")
        _bf16_cuda(resid, "resid")
        _req(resid.shape == (M, N) and resid.stride(1) == 1 and resid.stride(0) % 8 == 0 and resid.stride(0) >= N
             and resid.data_ptr() % 16 == 0, "bad resid")
        # in place is the same tensor; a resid that overlaps out any other way would be read after a write
        _req(resid.data_ptr() == out.data_ptr() and resid.stride(0) == out.stride(0)
             or not _overlap(resid, out), "resid may alias out only as the same rows")
        ldr = resid.stride(0)
    else:
        resid = None
    if M == 0:
        return out
    _check(lib().da_gemm_fp8(_ptr(aq), aq.stride(0), _ptr(wq), _ptr(sa), _ptr(sw), _ptr(out), out.stride(0),
                             _ptr(bias), _ptr(resid), ldr, M, N, K, epi, _stream()), "gemm_fp8")
    return out


def _overlap(a, b) -> bool:
    """True when the byte ranges spanned by two row-major 2-D tensors intersect."""
    def span(t):
        n = (t.shape[0] - 1) * t.stride(0) + t.shape[1] if t.numel() else 0
        return t.data_ptr(), t.data_ptr() + n * t.element_size()
    (a0, a1), (b0, b1) = span(a), span(b)
    return a0 < b1 and b0 < a1


def gemm_resid_norm(a, w, resid, gamma, eps: float, out=None, h_out=None, bias=None, tile: int = 0, splits: int = 0):
    """Decode layer tail (M <= 128): out = resid + a @ w^T (+ bias) — the new residual stream — and
    h_out = RMSNorm(out) * gamma, with the norm fused into the split-K reduction. Returns h_out."""
    _bf16_cuda(a, "a"); _bf16_cuda(w, "w"); _bf16_cuda(resid, "resid"); _bf16_cuda(gamma, "gamma")
    M, K = a.shape
    N = w.shape[0]
    _req(M <= 128 and K % 64 == 0 and N % 8 == 0 and N <= 8192 and w.shape[1] == K, "gemm_resid_norm shape")
    _req(a.stride(1) == 1 and a.stride(0) % 8 == 0 and w.is_contiguous() and gamma.numel() == N, "layout")
    _req(resid.shape == (M, N) and resid.stride(1) == 1, "bad resid")
    out = resid if out is None else out
    if h_out is None:
        h_out = torch.empty((M, N), dtype=torch.bfloat16, device=a.device)
    if M == 0:
        return h_out
    p = gemm_plan.plan_resid_norm(M, N, K, tile, splits)
    ws = _workspace(p.ws_bytes, a.device)
    _check(lib().da_gemm_resid_rmsnorm(_ptr(a), a.stride(0), _ptr(w), _ptr(out), out.stride(0), _ptr(bias),
                                       _ptr(resid), resid.stride(0), M, N, K, p.tile, p.splits, _ptr(ws), _ptr(gamma),
                                       float(eps), _ptr(h_out), h_out.stride(0), _stream()), "gemm_resid_norm")
    return h_out


# ------------------------------------------------------------------------------ norms etc.
def rmsnorm(x, w, eps: float, resid=None, out=None, route_m: int = 0):
    """route_m > M: run the kernel a pass over route_m rows would take (the many-row kernel sums a
    row's squares in another order), so a subset of that pass's rows gets the pass's bits."""
    _bf16_cuda(x, "x"); _bf16_cuda(w, "w")
    M, D = x.shape
    _req(x.stride(1) == 1 and x.stride(0) % 8 == 0, "x must be row-major")
    _row_d(D, "rmsnorm")
    _row_vec(w, D, torch.bfloat16, "w")
    if resid is not None:
        _bf16_cuda(resid, "resid"); _req(resid.is_contiguous() and resid.shape == (M, D), "resid must be [M, D]")
    if out is None:
        out = torch.empty((M, D), dtype=torch.bfloat16, device=x.device)
    _req(out.stride(1) == 1 and out.stride(0) % 8 == 0, "bad out")
    _check(lib().da_rmsnorm_routed(_ptr(x), x.stride(0), _ptr(resid), _ptr(w), _ptr(out), out.stride(0), M, D,
                                   float(eps), int(route_m), _stream()), "rmsnorm")
    return out


def rmsnorm_q8(x, g, eps: float, out=None, scale=None, route_m: int = 0):
    """RMSNorm straight to e4m3: (codes [M, D] float8_e4m3fn, scale [M] fp32), bit for bit
    quant_fp8(rmsnorm(x, g, eps, route_m=route_m)) in one pass that writes no bf16 row."""
    _bf16_cuda(x, "x"); _bf16_cuda(g, "g")
    _req(x.dim() == 2, "rmsnorm_q8 expects [M, D] rows")
    M, D = x.shape
    _req(x.stride(1) == 1 and x.stride(0) % 8 == 0 and x.stride(0) >= D and D % 8 == 0 and 0 < D <= 16384
         and x.data_ptr() % 16 == 0, "x must be row-major, D % 8 == 0, D <= 16384, 16-B aligned rows")
    _req(g.numel() == D and g.is_contiguous() and g.data_ptr() % 16 == 0, "g must be [D]")
    _req(eps > 0, "rmsnorm_q8 needs eps > 0")
    if out is None:
        out = torch.empty((M, D), dtype=FP8, device=x.device)
    if scale is None:
        scale = torch.empty(M, dtype=torch.float32, device=x.device)
    _req(out.is_cuda and out.dtype == FP8 and out.shape == (M, D) and out.stride(1) == 1 and out.stride(0) % 16 == 0
         and out.stride(0) >= D and out.data_ptr() % 16 == 0, "bad out")
    _req(scale.is_cuda and scale.dtype == torch.float32 and scale.is_contiguous() and scale.numel() >= M, "bad scale")
    _check(lib().da_rmsnorm_q8(_ptr(x), x.stride(0), _ptr(g), _ptr(out), out.stride(0), _ptr(scale), M, D, float(eps),
                               int(route_m), _stream()), "rmsnorm_q8")
    return out, scale


def layernorm(x, g, b, eps: float, resid=None, out=None, fp8_out: bool = False):
    """LayerNorm; with ``fp8_out`` also returns the row-quantised e4m3 copy and its scales
    (fused: the row is quantised from registers) -> (y, yq, yscale)."""
    _bf16_cuda(x, "x")
    M, D = x.shape
    _req(x.is_contiguous(), "x must be contiguous")
    _row_d(D, "layernorm")
    if resid is not None:
        _bf16_cuda(resid, "resid"); _req(resid.is_contiguous() and resid.shape == x.shape, "bad resid")
    _row_vec(g, D, torch.bfloat16, "g")
    if b is not None:
        _row_vec(b, D, torch.bfloat16, "b")
    if out is None:
        out = torch.empty_like(x)
    _row_out(out, M, D, torch.bfloat16, "out")
    if fp8_out:
        yq = torch.empty((M, D), dtype=FP8, device=x.device)
        ys = torch.empty(M, dtype=torch.float32, device=x.device)
        _check(lib().da_layernorm_q(_ptr(x), _ptr(resid), _ptr(g), _ptr(b), _ptr(out), _ptr(yq), _ptr(ys), M, D,
                                    float(eps), _stream()), "layernorm_q")
        return out, yq, ys
    _check(lib().da_layernorm(_ptr(x), _ptr(resid), _ptr(g), _ptr(b), _ptr(out), M, D, float(eps), _stream()),
           "layernorm")
    return out


def bert_embed_ln(ids, positions, types, word, pos, type_, g, b, eps: float, out=None, fp8_out: bool = False):
    _i32(ids, "ids"); _i32(positions, "positions")
    if types is not None:
        _i32(types, "types")
    T = ids.numel()
    _req(word.dim() == 2, "word must be [rows, D]")
    D = word.shape[1]
    _req(positions.numel() == T and (types is None or types.numel() == T), "positions / types length")
    _row_d(D, "bert_embed_ln")
    for t, n in ((word, "word"), (pos, "pos"), (type_, "type")):
        _row_table(t, D, torch.bfloat16, n)
    _row_vec(g, D, torch.bfloat16, "g"); _row_vec(b, D, torch.bfloat16, "b")
    if out is None:
        out = torch.empty((T, D), dtype=torch.bfloat16, device=ids.device)
    _row_out(out, T, D, torch.bfloat16, "out")
    if fp8_out:
        yq = torch.empty((T, D), dtype=FP8, device=ids.device)
        ys = torch.empty(T, dtype=torch.float32, device=ids.device)
        _check(lib().da_bert_embed_ln_q(_ptr(ids), _ptr(positions), _ptr(types), _ptr(word), _ptr(pos), _ptr(type_),
                                        _ptr(g), _ptr(b), _ptr(out), _ptr(yq), _ptr(ys), T, D, float(eps), _stream()),
               "bert_embed_ln_q")
        return out, yq, ys
    _check(lib().da_bert_embed_ln(_ptr(ids), _ptr(positions), _ptr(types), _ptr(word), _ptr(pos), _ptr(type_),
                                  _ptr(g), _ptr(b), _ptr(out), T, D, float(eps), _stream()), "bert_embed_ln")
    return out


def embed(ids, table, out=None):
    _i32(ids, "ids"); _bf16_cuda(table, "table")
    _req(table.dim() == 2, "table must be [rows, D]")
    T, D = ids.numel(), table.shape[1]
    _row_d(D, "embed")
    _row_table(table, D, torch.bfloat16, "table")
    if out is None:
        out = torch.empty((T, D), dtype=torch.bfloat16, device=ids.device)
    _row_out(out, T, D, torch.bfloat16, "out")
    _check(lib().da_embed(_ptr(ids), _ptr(table), _ptr(out), T, D, _stream()), "embed")
    return out


def pool_l2norm(h, cu_seqlens, mode: int = 0, out32=None, out16=None):
    _bf16_cuda(h, "h"); _i32(cu_seqlens, "cu_seqlens")
    B = cu_seqlens.numel() - 1
    _req(h.dim() == 2 and h.is_contiguous() and B >= 0, "h must be contiguous [T, D]")
    D = h.shape[1]
    _row_d(D, "pool_l2norm")
    if out32 is None and out16 is None:
        out32 = torch.empty((B, D), dtype=torch.float32, device=h.device)
    _pool_outs(B, D, out32, out16)
    _check(lib().da_pool_l2norm(_ptr(h), _ptr(cu_seqlens), B, D, mode, _ptr(out32), _ptr(out16), _stream()),
           "pool_l2norm")
    return out32 if out32 is not None else out16


def rope_cache(qkv, pos, cos_sin, H, Hkv, D, slot=None, k_cache=None, v_cache=None, rotate_q=True):
    """In-place RoPE on q and k heads of qkv [T, (H+2Hkv)*D]; optionally writes k/v into the cache."""
    _bf16_cuda(qkv, "qkv"); _i32(pos, "pos")
    T = qkv.shape[0]
    _req(qkv.is_contiguous() and qkv.shape[1] == (H + 2 * Hkv) * D, "qkv shape")
    _req(cos_sin.dtype == torch.float32 and cos_sin.is_contiguous() and cos_sin.shape[-1] == 2
         and cos_sin.shape[1] == D // 2, "cos_sin must be fp32 [max_pos, D/2, 2]")
    max_seq = 0
    if k_cache is not None:
        _i32(slot, "slot")
        _req(k_cache.is_contiguous() and v_cache.is_contiguous() and k_cache.shape == v_cache.shape, "caches")
        _req(k_cache.dim() == 4 and k_cache.shape[1] == Hkv and k_cache.shape[3] == D, "cache [S, Hkv, max_seq, D]")
        max_seq = k_cache.shape[2]
    _check(lib().da_rope_cache(_ptr(qkv), _ptr(pos), _ptr(slot), _ptr(cos_sin), _ptr(k_cache), _ptr(v_cache),
                               T, H, Hkv, D, max_seq, 1 if rotate_q else 0, _stream()), "rope_cache")
    return qkv


def flash_kv_cache_ok(D: int, causal: bool) -> bool:
    """True when flash_attn_varlen can read the sequences' own keys from the KV cache (kv_cache=)."""
    return causal and D == 96


def flash_attn_varlen(q, k, v, cu_seqlens, max_seqlen: int, H: int, Hkv: int, D: int, causal: bool,
                      scale: float | None = None, out=None, prefix=None, kv_cache=None, tail_only: bool = False):
    """q/k/v: 2-D [T, *] views with head h at columns h*D (strided views into a packed qkv are fine).
    prefix = (k_pre, v_pre, P): shared-prefix keys of every sequence, one KV-cache slot's
    [Hkv, max_seq, D] K and V (RoPE applied); query i of a sequence is key P + i.
    kv_cache = (k_cache, v_cache, slot, pos) (flash_kv_cache_ok only): the own keys of the sequence
    starting at token t are k_cache[slot[t], :, pos[t] + j] (slot / pos int32 per token, as the QKV
    projection wrote them); k / v are then ignored (None allowed).
    tail_only: per (sequence, head) only the query block that holds the sequence's last token is
    computed and stored (one workgroup; the same bits as a full launch gives those rows); every other
    row of ``out`` is left as it was."""
    kc = vc = ks = kpos = None
    if kv_cache is not None:
        kc, vc, ks, kpos = kv_cache
        _req(flash_kv_cache_ok(D, causal), "kv_cache: causal D = 96 only")
        _bf16_cuda(kc, "k_cache"); _bf16_cuda(vc, "v_cache"); _i32(ks, "slot"); _i32(kpos, "pos")
        _req(kc.is_contiguous() and vc.is_contiguous() and kc.shape == vc.shape and kc.dim() == 4
             and kc.shape[1] == Hkv and kc.shape[3] == D, "caches [slots, Hkv, max_seq, D]")
        _req(ks.numel() >= q.shape[0] and kpos.numel() >= q.shape[0], "slot / pos per token")
        k = v = q  # unused by the kernel in this mode
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        _bf16_cuda(t, n)
        _req(t.dim() == 2 and t.stride(1) == 1 and t.stride(0) % 8 == 0 and t.data_ptr() % 16 == 0, f"{n} layout")
    _i32(cu_seqlens, "cu_seqlens")
    _req(D in (32, 64, 96, 128), f"head dim {D} unsupported")
    _req(H % Hkv == 0, "H % Hkv")
    T = q.shape[0]
    if out is None:
        out = torch.empty((T, H * D), dtype=torch.bfloat16, device=q.device)
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    B = cu_seqlens.numel() - 1
    kp = vp = None
    hstride, P = 0, 0
    if prefix is not None:
        kp, vp, P = prefix
        P = int(P)
        _bf16_cuda(kp, "k_pre"); _bf16_cuda(vp, "v_pre")
        _req(kp.dim() == 3 and kp.shape == vp.shape and kp.shape[0] == Hkv and kp.shape[2] == D
             and kp.is_contiguous() and vp.is_contiguous() and 0 <= P <= kp.shape[1], "prefix K/V [Hkv, max_seq, D]")
        hstride = kp.shape[1] * D
    if kc is not None:
        _req(prefix is None or kp.shape[1] == kc.shape[2], "prefix and caches differ in max_seq")
        hstride = kc.shape[2] * D
    _check(lib().da_flash_attn_v2(_ptr(q), _ptr(k), _ptr(v), q.stride(0), k.stride(0), v.stride(0),
                                  _ptr(cu_seqlens), B, int(max_seqlen), H, Hkv, D, int(causal), float(scale),
                                  _ptr(out), out.stride(0), _ptr(kp), _ptr(vp), hstride, P, _ptr(ks), _ptr(kpos),
                                  _ptr(kc), _ptr(vc), int(bool(tail_only)), _stream()),
           "flash_attn_varlen")
    return out


# Split-KV partials merged inside the decode kernel by the last split of each (row, kv head)
# (False: separate combine launch; tests cover both). The ticket counters stay zero between
# launches; buffers are only ever added, never freed, so a captured graph's pointer stays valid.
_FUSED_COMBINE = True
_UC: dict = {}


class _RawBuf:
    """A device allocation outside PyTorch's allocator (uncached memory), as a ``_ptr``-able object."""

    def __init__(self, ptr: int, nbytes: int):
        self.ptr, self.nbytes = ptr, nbytes

    def data_ptr(self) -> int:
        return self.ptr


def _uncached(tag: str, nbytes: int, device) -> _RawBuf:
    """Zeroed uncached (L2-bypassing) device memory for cross-workgroup hand-offs (decode split
    partials + tickets). Grows by adding buffers, never frees: captured graphs keep their pointers."""
    key = (tag, device.index if device.index is not None else torch.cuda.current_device(),
           getattr(_ROLE, "name", "main"))
    bufs = _UC.setdefault(key, [])
    if not bufs or bufs[-1].nbytes < nbytes:
        n = max(nbytes, 1 << 20)
        p = ctypes.c_void_p()
        with torch.cuda.device(device):
            _check(lib().da_malloc_uncached(n, ctypes.byref(p)), "hipExtMallocWithFlags(uncached)")
        bufs.append(_RawBuf(p.value, n))
    return bufs[-1]


def _decode_split(B: int, Hkv: int, max_len: int, chunk: int):
    """(chunk, nsplit) of a decode-attention launch (static for a captured graph: from max_len)."""
    if chunk <= 0:
        # measured on MI355X (profiles/decode_attn_chunks_r1.txt): per-workgroup overhead dominates
        # small chunks; aim for ~768 workgroups, 512..4096 keys each
        want = max_len * B * Hkv / 768
        chunk = 512
        while chunk < want and chunk < 4096:
            chunk *= 2
    return chunk, max(1, math.ceil(max_len / chunk))


# Same-XCD split exchange of the batch-1..small-batch MHA decode attention (decode_attn.hip, DEC_XC):
# all splits of a (row, kv head) pair on one XCD, their partials and ticket in cached memory (L2
# round trips instead of uncached ones). It relies on the launch's workgroup -> XCD round-robin, so
# it is used only after the placement probe confirmed that on this device, and never once a
# CU-masked stream exists in the process (a masked queue need not dispatch round-robin over XCDs;
# ops/streams.py sets MASKED_STREAMS). DA_DECODE_XC=0 turns it off.
DECODE_XC = os.environ.get("DA_DECODE_XC", "1") != "0"
MASKED_STREAMS = False
_XC_PROBE: dict = {}


def decode_xc_ok(device) -> bool:
    """True when every workgroup w of a launch runs on XCD w % 8 here (placement probe, once per
    device; not during a graph capture, where the answer stays unknown = False)."""
    if not DECODE_XC or MASKED_STREAMS:
        return False
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx in _XC_PROBE:
        return _XC_PROBE[idx]
    if torch.cuda.is_current_stream_capturing():
        return False
    n = 1024
    out = torch.zeros(n * 4, dtype=torch.int32, device=device)
    _check(lib().da_placement_probe(_ptr(out), n, 0, _stream()), "placement_probe")
    xcc = out.view(n, 4)[:, 0].cpu().numpy()
    ok = bool(len(set(xcc.tolist())) == 8 and all(len(set(xcc[r::8].tolist())) == 1 for r in range(8)))
    _XC_PROBE[idx] = ok
    return ok


_COUNTERS: dict = {}


def _cached_counters(tag: str, n: int, device) -> torch.Tensor:
    """Zeroed int32 counters in ordinary device memory that stay allocated (captured graphs keep the
    pointer; the kernels leave them zero)."""
    key = (tag, device.index if device.index is not None else torch.cuda.current_device(),
           getattr(_ROLE, "name", "main"))  # per workspace role, like the uncached ones: concurrent lanes
    bufs = _COUNTERS.setdefault(key, [])
    if not bufs or bufs[-1].numel() < n:
        bufs.append(torch.zeros(max(n, 1024), dtype=torch.int32, device=device))
    return bufs[-1]


def _decode_operands(q, lens, slot, H, Hkv, D, max_len, max_seq, chunk, out, pre, rope=None):
    """The operand checks of both decode wrappers (the cache's own are the caller's; max_seq = its
    capacity). Returns (chunk, nsplit, out, cos_sin, pos)."""
    _bf16_cuda(q, "q"); _i32(lens, "lens"); _i32(slot, "slot")
    _req(D in (64, 96, 128), "head dim")
    _req(H % Hkv == 0 and (H // Hkv) in (1, 2, 4, 8), "GQA group must be 1/2/4/8")
    _req(q.dim() == 2 and q.stride(1) == 1 and q.shape[1] >= H * D, "q [B, >= H*D]")
    B = q.shape[0]
    _req(lens.numel() >= B and slot.numel() >= B, "lens / slot length")
    _req(0 < max_len <= max_seq, "max_len > cache capacity")
    if pre is not None:
        _i32(pre, "pre"); _req(pre.shape == (B, 2) and pre.is_contiguous(), "pre must be int32 [B, 2]")
    cs = ps = None
    if rope is not None:
        cs, ps = rope
        _req(H == Hkv and D % 8 == 0, "fused RoPE decode: MHA only")
        _i32(ps, "pos")
        _req(cs.dtype == torch.float32 and cs.is_contiguous() and cs.shape[1] == D // 2 and cs.shape[2] == 2, "cos_sin")
        _req(q.shape[1] >= (H + 2 * Hkv) * D, "fused RoPE decode needs the qkv row")
    chunk, nsplit = _decode_split(B, Hkv, max_len, chunk)
    _req(chunk % 64 == 0, "chunk must be a multiple of 64")
    if out is None:
        out = torch.empty((B, H * D), dtype=torch.bfloat16, device=q.device)
    _bf16_cuda(out, "out")
    _req(out.dim() == 2 and out.shape[0] == B and out.shape[1] >= H * D and out.stride(1) == 1, "out [B, >= H*D]")
    return chunk, nsplit, out, cs, ps


def _decode_buffers(B, H, Hkv, D, nsplit, device, same_xcd_ok: bool):
    """(ws, cnt, xc) of a launch: the split partials and, when the kernel merges them itself, the
    tickets — in uncached memory, or (xc = 1, bf16 cache only: same_xcd_ok) in cached memory with all
    splits of a (row, kv head) pair on one XCD. No tickets: a combine launch merges."""
    nws = B * H * nsplit * (D + 2) * 4
    ws = _workspace(nws, device)
    if not (_FUSED_COMBINE and nsplit > 1):
        return ws, None, 0
    if same_xcd_ok and H == Hkv and B * Hkv <= 32 and (B * Hkv) % 8 == 0 and decode_xc_ok(device):
        return ws, _cached_counters("decode_cnt_xc", B * Hkv, device), 1  # the role workspace: cached memory
    cnt = _uncached("decode_cnt", B * Hkv * 4, device)
    return _uncached("decode_ws", nws, device), cnt, 0


def decode_attn(q, k_cache, v_cache, lens, slot, H, Hkv, D, max_len: int, chunk: int = 0, scale=None, out=None,
                pre=None, rope=None):
    """q [B, >=H*D] (row stride any multiple of 8); lens/slot int32 [B]; max_len = max(lens) or the
    cache capacity (host int, fixes the split count so the launch is graph-capturable).
    chunk = keys per workgroup (0 = auto: enough workgroups to fill 256 CUs, 4 waves x 64-key tiles).
    pre: optional int32 [B, 2] device tensor (P, prefix slot), 0 <= P <= lens: keys [0, P) of row b
    are the batch's shared prompt head, stored once in the prefix slot (read through the cache; any P,
    whole 64-key tiles being the form the decoder uses).
    rope = (cos_sin fp32 [max_pos, D/2, 2], pos int32 [B]), MHA only: q is the raw qkv row
    [B, (H + 2 Hkv) D]; the kernel applies RoPE to q and the new token's k and writes that token's
    k / v into the cache at pos (== lens - 1) — the decode step's rope_cache launch folded in."""
    _req(k_cache.dim() == 4 and k_cache.shape[1] == Hkv and k_cache.shape[3] == D, "cache shape")
    _req(rope is None or (k_cache.is_contiguous() and v_cache.is_contiguous()), "caches must be contiguous")
    chunk, nsplit, out, cs, ps = _decode_operands(q, lens, slot, H, Hkv, D, max_len, k_cache.shape[2], chunk, out, pre,
                                                  rope)
    B = q.shape[0]
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    ws, cnt, xc = _decode_buffers(B, H, Hkv, D, nsplit, q.device, same_xcd_ok=True)
    _check(lib().da_decode_attn(_ptr(q), q.stride(0), _ptr(k_cache), _ptr(v_cache), _ptr(lens), _ptr(slot), _ptr(pre), B, H,
                                Hkv, D, k_cache.shape[2], chunk, nsplit, float(scale), _ptr(ws), _ptr(out), out.stride(0),
                                _ptr(cnt), _ptr(cs), _ptr(ps), xc, _stream()), "decode_attn")
    return out


# ----------------------------------------------------------------------------------- fp8 KV cache
def _kv8_cache_checks(k_codes, v_codes, k_scale, v_scale, Hkv, D):
    for c, s, n in ((k_codes, k_scale, "k"), (v_codes, v_scale, "v")):
        _req(c.is_cuda and c.dtype in (FP8, torch.uint8) and c.is_contiguous(), f"{n}_codes must be contiguous e4m3 on GPU")
        _req(c.dim() == 4 and c.shape[1] == Hkv and c.shape[3] == D, f"{n}_codes [slots, Hkv, max_seq, D]")
        _req(s.is_cuda and s.dtype == torch.float32 and s.is_contiguous() and s.shape == c.shape[:3],
             f"{n}_scale must be contiguous fp32 [slots, Hkv, max_seq]")
        _req(c.data_ptr() % 16 == 0 and s.data_ptr() % 4 == 0, f"{n} cache alignment")
    _req(k_codes.shape == v_codes.shape, "k / v caches differ in shape")


def rope_cache_kv8(qkv, pos, cos_sin, H, Hkv, D, slot, k_codes, v_codes, k_scale, v_scale, rotate_q=True):
    """In-place RoPE on the q and k heads of qkv [T, (H+2Hkv)*D] (the roundings of rope_cache), then
    the rotated k row and the v row of every (token, kv head) quantised to e4m3 with one power-of-two
    scale per row (quant_weight_fp8_pow2's rule) and written to the fp8 cache at [slot[t], :, pos[t]]
    (codes [slots, Hkv, max_seq, D], scales fp32 [slots, Hkv, max_seq]). pos[t] < max_seq and
    0 <= slot[t] < slots are the caller's contract, as for rope_cache."""
    _bf16_cuda(qkv, "qkv"); _i32(pos, "pos"); _i32(slot, "slot")
    T = qkv.shape[0]
    _req(D in (64, 96, 128), "head dim")
    _req(qkv.is_contiguous() and qkv.shape[1] == (H + 2 * Hkv) * D and qkv.data_ptr() % 16 == 0, "qkv shape")
    _req(pos.numel() >= T and slot.numel() >= T, "pos / slot length")
    _req(cos_sin.is_cuda and cos_sin.dtype == torch.float32 and cos_sin.is_contiguous() and cos_sin.dim() == 3
         and cos_sin.shape[-1] == 2 and cos_sin.shape[1] == D // 2, "cos_sin must be fp32 [max_pos, D/2, 2]")
    _kv8_cache_checks(k_codes, v_codes, k_scale, v_scale, Hkv, D)
    _check(lib().da_rope_cache_kv8(_ptr(qkv), _ptr(pos), _ptr(slot), _ptr(cos_sin), _ptr(k_codes), _ptr(v_codes),
                                   _ptr(k_scale), _ptr(v_scale), T, H, Hkv, D, k_codes.shape[2],
                                   1 if rotate_q else 0, _stream()), "rope_cache_kv8")
    return qkv


def decode_attn_kv8(q, k_codes, v_codes, k_scale, v_scale, lens, slot, H, Hkv, D, max_len: int, chunk: int = 0,
                    scale=None, out=None, pre=None):
    """decode_attn (without rope=) over the fp8 cache: q [B, >= H*D] bf16 (any row stride), lens / slot
    int32 [B], max_len fixes the split count (graph-capturable), pre int32 [B, 2] = (P, prefix slot)
    with 0 <= P <= lens, out bf16 with any row stride. Splits merge in the kernel through the uncached
    workspace and ticket (or a combine launch with _FUSED_COMBINE off); never the same-XCD exchange."""
    _kv8_cache_checks(k_codes, v_codes, k_scale, v_scale, Hkv, D)
    chunk, nsplit, out, _, _ = _decode_operands(q, lens, slot, H, Hkv, D, max_len, k_codes.shape[2], chunk, out, pre)
    B = q.shape[0]
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    ws, cnt, _ = _decode_buffers(B, H, Hkv, D, nsplit, q.device, same_xcd_ok=False)
    _check(lib().da_decode_attn_kv8(_ptr(q), q.stride(0), _ptr(k_codes), _ptr(v_codes), _ptr(k_scale), _ptr(v_scale),
                                    _ptr(lens), _ptr(slot), _ptr(pre), B, H, Hkv, D, k_codes.shape[2], chunk, nsplit,
                                    float(scale), _ptr(ws), _ptr(out), out.stride(0), _ptr(cnt), _stream()),
           "decode_attn_kv8")
    return out


def kv8_dequant(codes, scale, slot: int, P: int):
    """bf16 [Hkv, P, D]: the first P keys of cache slot ``slot`` (host int) dequantised, exactly — the
    shared prefix the flash prefill reads in bf16."""
    slot, P = int(slot), int(P)
    _req(codes.is_cuda and codes.dtype in (FP8, torch.uint8) and codes.is_contiguous() and codes.dim() == 4
         and codes.shape[3] % 16 == 0 and codes.data_ptr() % 16 == 0, "codes [slots, Hkv, max_seq, D]")
    _req(scale.is_cuda and scale.dtype == torch.float32 and scale.is_contiguous() and scale.shape == codes.shape[:3],
         "scale fp32 [slots, Hkv, max_seq]")
    S, Hkv, max_seq, D = codes.shape
    _req(0 <= slot < S and 0 <= P <= max_seq, "slot / P out of range")
    out = torch.empty((Hkv, P, D), dtype=torch.bfloat16, device=codes.device)
    _check(lib().da_kv8_dequant(_ptr(codes), _ptr(scale), slot, S, Hkv, P, D, max_seq, _ptr(out), _stream()),
           "kv8_dequant")
    return out


# rows up to which sample() cuts the vocabulary over many workgroups (0: always one per row); at
# batch 64 one workgroup per row leaves 192 CUs idle too
SAMPLE_CHUNKED_MAX_B = 64
_SAMPLE_WS: dict = {}


def _sample_ws(nfloats: int, device) -> torch.Tensor:
    """Per-(device, workspace role) fp32 scratch of the chunked sampler. Grows by adding buffers and
    never frees one: a captured decode graph keeps pointing at the buffer it was captured with."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), getattr(_ROLE, "name", "main"))
    bufs = _SAMPLE_WS.setdefault(key, [])
    if not bufs or bufs[-1].numel() < nfloats:
        bufs.append(torch.empty(max(nfloats, 16384), dtype=torch.float32, device=device))
    return bufs[-1]


def sample(logits, temperature: float, seed: int, step: int = 0, out_tok=None, out_lp=None, conf=None,
           active=None, ctr=None, pos=None, lens=None, hist=None, start=None, eos=()):
    """Fused temperature sampler (see rope_sample.hip). Returns (tokens, logprobs)."""
    _bf16_cuda(logits, "logits")
    B, V = logits.shape
    _req(logits.stride(1) == 1 and logits.stride(0) % 8 == 0, "logits layout")
    dev = logits.device
    if out_tok is None:
        out_tok = torch.empty(B, dtype=torch.int32, device=dev)
    if out_lp is None:
        out_lp = torch.empty(B, dtype=torch.float32, device=dev)
    if conf is not None:
        _req(conf.dtype == torch.float32 and conf.shape == (B, 2), "conf must be fp32 [B, 2]")
    for t, n in ((active, "active"), (ctr, "ctr"), (pos, "pos"), (lens, "lens"), (start, "start")):
        if t is not None:
            _i32(t, n); _req(t.numel() >= B, f"{n} too short")
    hist_ld = 0
    if hist is not None:
        _i32(hist, "hist"); _req(hist.dim() == 2 and hist.shape[0] >= B, "hist [B, n]")
        _req(pos is not None and start is not None, "hist needs pos and start")
        hist_ld = hist.shape[1]
    e = list(eos)[:4] + [-1] * (4 - min(4, len(eos)))
    if B <= SAMPLE_CHUNKED_MAX_B and V >= 4096:
        # few rows: the row is split over ceil(V / 1024) workgroups + a finalize launch (same token;
        # the batch-1 sampler took ~21 us on one CU, rope_sample.hip sample_chunk_kernel)
        ws = _sample_ws(B * ((V + 1023) // 1024) * 8, dev)
        _check(lib().da_sample_chunked(_ptr(logits), B, V, logits.stride(0), float(temperature), seed & 0xffffffff,
                                       step & 0xffffffff, _ptr(ctr), _ptr(ws), _ptr(out_tok), _ptr(out_lp),
                                       _ptr(conf), _ptr(active), _ptr(pos), _ptr(lens), _ptr(hist), _ptr(start),
                                       hist_ld, e[0], e[1], e[2], e[3], _stream()), "sample_chunked")
        return out_tok, out_lp
    _check(lib().da_sample(_ptr(logits), B, V, logits.stride(0), float(temperature), seed & 0xffffffff,
                           step & 0xffffffff, _ptr(ctr), _ptr(out_tok), _ptr(out_lp), _ptr(conf), _ptr(active),
                           _ptr(pos), _ptr(lens), _ptr(hist), _ptr(start), hist_ld, e[0], e[1], e[2], e[3],
                           _stream()), "sample")
    return out_tok, out_lp


def sample_partial(logits, temperature: float, seed: int, v0: int, step: int = 0, ctr=None, out=None):
    """Vocab-parallel sampling, rank side: logits [B, Vl] of the vocabulary slice starting at global
    index v0 -> stats fp32 [B, 8] = (best Gumbel score, best global index as int bits, local max,
    local sum exp(x - max), logit of the best, 0, 0, 0). See rope_sample.hip."""
    _bf16_cuda(logits, "logits")
    B, V = logits.shape
    _req(logits.stride(1) == 1, "logits rows must be contiguous")
    if ctr is not None:
        _i32(ctr, "ctr"); _req(ctr.numel() >= B, "ctr too short")
    if out is None:
        out = torch.empty((B, 8), dtype=torch.float32, device=logits.device)
    _req(out.dtype == torch.float32 and out.shape == (B, 8) and out.is_contiguous(), "stats must be fp32 [B, 8]")
    _check(lib().da_sample_partial(_ptr(logits), B, V, logits.stride(0), int(v0), float(temperature),
                                   seed & 0xffffffff, step & 0xffffffff, _ptr(ctr), _ptr(out), _stream()),
           "sample_partial")
    return out


def sample_finalize(gathered, ranks: int, out_tok=None, out_lp=None, conf=None, active=None, pos=None, lens=None,
                    hist=None, start=None, eos=()):
    """Vocab-parallel sampling, merge side: gathered fp32 [B, ranks * 8] (every rank's stats, rank
    order) -> the token / logprob / bookkeeping of ``sample`` on the full row."""
    _req(gathered.is_cuda and gathered.dtype == torch.float32 and gathered.is_contiguous(), "gathered fp32")
    B = gathered.shape[0]
    _req(gathered.shape == (B, 8 * ranks), f"gathered must be [B, {8 * ranks}]")
    dev = gathered.device
    if out_tok is None:
        out_tok = torch.empty(B, dtype=torch.int32, device=dev)
    if out_lp is None:
        out_lp = torch.empty(B, dtype=torch.float32, device=dev)
    if conf is not None:
        _req(conf.dtype == torch.float32 and conf.shape == (B, 2), "conf must be fp32 [B, 2]")
    for t, n in ((active, "active"), (pos, "pos"), (lens, "lens"), (start, "start")):
        if t is not None:
            _i32(t, n); _req(t.numel() >= B, f"{n} too short")
    hist_ld = 0
    if hist is not None:
        _i32(hist, "hist"); _req(hist.dim() == 2 and hist.shape[0] >= B, "hist [B, n]")
        _req(pos is not None and start is not None, "hist needs pos and start")
        hist_ld = hist.shape[1]
    e = list(eos)[:4] + [-1] * (4 - min(4, len(eos)))
    _check(lib().da_sample_finalize(_ptr(gathered), B, ranks, _ptr(out_tok), _ptr(out_lp), _ptr(conf), _ptr(active),
                                    _ptr(pos), _ptr(lens), _ptr(hist), _ptr(start), hist_ld, e[0], e[1], e[2], e[3],
                                    _stream()), "sample_finalize")
    return out_tok, out_lp


# --------------------------------------------------------------------------- vector search
def topk_dense(X, Qv, K: int, thr: float, slots=None, bitmap=None, rows_per_block: int | None = None):
    """Exact top-K of Qv @ X^T per query with threshold and optional doc-slot bitmap [Q, W] int32."""
    _bf16_cuda(X, "X"); _bf16_cuda(Qv, "Qv")
    N, d = X.shape
    Q = Qv.shape[0]
    _req(X.is_contiguous() and Qv.is_contiguous() and Qv.shape[1] == d, "X/Qv layout")
    _req(d % 32 == 0 and 1 <= K <= 32, "d % 32 and 1 <= K <= 32")
    W = 0
    if slots is not None:
        _i32(slots, "slots")
        _req(slots.numel() >= N, "slots length")
    if bitmap is not None:
        _req(slots is not None, "bitmap needs slots")
        _req(bitmap.dtype == torch.int32 and bitmap.is_contiguous() and bitmap.shape[0] == Q, "bitmap [Q, W] int32")
        W = bitmap.shape[1]
    if d in (384, 768, 1024) and rows_per_block is None and N > 0 and Q <= 256:
        # the streaming scan (search-sized batches over a big shard; k-means assignment, with the
        # rows as the queries, keeps the query-major tiles below): ~16 waves of rows per CU over
        # the chip (256 CUs), >= 64 rows each
        rpw = max(64, math.ceil(N / (256 * 16) / 16) * 16)
        ws = _workspace(int(lib().da_topk_stream_ws(N, Q, K, rpw)), X.device)
        out_s = torch.empty((Q, K), dtype=torch.float32, device=X.device)
        out_i = torch.empty((Q, K), dtype=torch.int32, device=X.device)
        _check(lib().da_topk_dense_stream(_ptr(X), N, d, _ptr(slots), _ptr(Qv), Q, _ptr(bitmap), W, float(thr), K,
                                          rpw, _ptr(ws), _ptr(out_s), _ptr(out_i), _stream()), "topk_dense_stream")
        return out_s, out_i
    if rows_per_block is None:
        qt = math.ceil(Q / 16)
        nblk = max(1, min(math.ceil(N / 256), max(1, 1024 // qt)))
        rows_per_block = max(64, math.ceil(math.ceil(N / nblk) / 64) * 64)
    nblk = max(1, math.ceil(N / rows_per_block))
    ws = _workspace(nblk * Q * K * 8, X.device)
    out_s = torch.empty((Q, K), dtype=torch.float32, device=X.device)
    out_i = torch.empty((Q, K), dtype=torch.int32, device=X.device)
    _check(lib().da_topk_dense(_ptr(X), N, d, _ptr(slots), _ptr(Qv), Q, _ptr(bitmap), W, float(thr), K,
                               rows_per_block, _ptr(ws), _ptr(out_s), _ptr(out_i), _stream()), "topk_dense")
    return out_s, out_i


def topk_ranges(X, Qv, ranges, range_off, K: int, thr: float, max_rows: int, slots=None, bitmap=None,
                rows_per_split: int = 512):
    """Top-K per query over its own row ranges. ranges int32 [R, 2], range_off int32 [Q+1];
    max_rows = max total rows of any query (host int) — sets the split count."""
    _bf16_cuda(X, "X"); _bf16_cuda(Qv, "Qv")
    N, d = X.shape
    Q = Qv.shape[0]
    _req(d % 8 == 0 and d <= 4096 and 1 <= K <= 32, "d / K limits")
    _i32(ranges, "ranges"); _i32(range_off, "range_off")
    _req(range_off.numel() == Q + 1, "range_off length")
    W = 0
    if slots is not None:
        _i32(slots, "slots")
        _req(slots.numel() >= N, "slots length")
    if bitmap is not None:
        _req(slots is not None, "bitmap needs slots")
        _req(bitmap.dtype == torch.int32 and bitmap.shape[0] == Q, "bitmap")
        W = bitmap.shape[1]
    splits = max(1, math.ceil(max_rows / rows_per_split))
    ws = _workspace(splits * Q * K * 8, X.device)
    out_s = torch.empty((Q, K), dtype=torch.float32, device=X.device)
    out_i = torch.empty((Q, K), dtype=torch.int32, device=X.device)
    _check(lib().da_topk_ranges(_ptr(X), d, _ptr(slots), _ptr(Qv), Q, _ptr(ranges), _ptr(range_off), _ptr(bitmap),
                                W, float(thr), K, splits, rows_per_split, _ptr(ws), _ptr(out_s), _ptr(out_i),
                                _stream()), "topk_ranges")
    return out_s, out_i


# ------------------------------------------------------------------- fp8 vector index (INDEX_DTYPE=fp8)
# rows as e4m3 codes [N, d] (uint8 or float8_e4m3fn) + one fp32 power-of-two scale per row
# (quant_weight_fp8_pow2's rule); queries stay bf16. See csrc/vecsearch8.hip.
DENSE8_DIMS = (128, 384, 768, 1024)  # the widths the fp8 dense scan is built for


def _codes_cuda(codes, scale, rows: int):
    _req(codes.is_cuda and codes.dtype in (FP8, torch.uint8) and codes.dim() == 2 and codes.is_contiguous(),
         "codes must be contiguous e4m3 / uint8 [N, d] on GPU")
    _req(scale.is_cuda and scale.dtype == torch.float32 and scale.dim() == 1 and scale.is_contiguous()
         and scale.numel() >= rows, "scale must be contiguous fp32 [>= N] on GPU")
    _req(codes.data_ptr() % 16 == 0, "codes alignment")


def _row_index(t, name: str, n: int, cap: int):
    """An int64 [n] row list on the GPU with every entry inside [0, cap) (read back: one host sync)."""
    _req(t.is_cuda and t.dtype == torch.int64 and t.dim() == 1 and t.is_contiguous() and t.numel() == n,
         f"{name} must be contiguous int64 [{n}] on GPU")
    if n:
        lo, hi = torch.aminmax(t)
        _req(int(lo) >= 0 and int(hi) < cap, f"{name} names rows outside [0, {cap})")


def index_quant_rows(X, codes, scale, row0: int = 0, dest=None):
    """bf16 rows X [n, d] -> codes[row0:row0 + n] (uint8 / e4m3 [cap, d]) and scale[row0:row0 + n]
    (fp32 [cap]), bit-identical to reference.quant_weight_fp8_pow2(X). Nothing else is written.
    ``dest`` (int64 [n], distinct rows inside codes; row0 must be 0): row r goes to codes[dest[r]],
    scale[dest[r]] instead (the IVF streaming build's scatter pass)."""
    _bf16_cuda(X, "X")
    _req(X.dim() == 2 and X.is_contiguous() and X.data_ptr() % 8 == 0, "X must be contiguous [n, d]")
    n, d = X.shape
    row0 = int(row0)
    if dest is not None:
        _req(row0 == 0, "dest and row0 exclude each other")
        _codes_cuda(codes, scale, codes.shape[0])
        _req(d % 4 == 0 and codes.shape[1] == d, "d % 4 == 0 and codes [cap, d]")
        _row_index(dest, "dest", n, codes.shape[0])
        _check(lib().da_index_quant_scatter(_ptr(X), n, d, _ptr(codes), _ptr(scale), _ptr(dest), codes.shape[0],
                                            _stream()), "index_quant_scatter")
        return codes, scale
    _codes_cuda(codes, scale, row0 + n)
    _req(d % 4 == 0 and codes.shape[1] == d, "d % 4 == 0 and codes [cap, d]")
    _req(0 <= row0 and row0 + n <= codes.shape[0], "rows [row0, row0 + n) outside codes")
    _check(lib().da_index_quant_rows(_ptr(X), n, d, _ptr(codes), _ptr(scale), row0, _stream()), "index_quant_rows")
    return codes, scale


def index_dequant_rows(codes, scale, out, row0: int = 0, sel=None):
    """bf16 out [n, d] <- codes[r] * scale[r] (exact) for rows row0 .. row0 + n of the store, or for the
    rows ``sel`` (int64 [n], repeats allowed; row0 must be 0): bit-identical to reference.index_dequant
    of those rows. Nothing outside ``out`` is written."""
    _bf16_cuda(out, "out")
    _req(out.dim() == 2 and out.is_contiguous() and out.data_ptr() % 16 == 0, "out must be contiguous [n, d]")
    n, d = out.shape
    row0 = int(row0)
    cap = codes.shape[0]
    _codes_cuda(codes, scale, cap)
    _req(d % 16 == 0 and d >= 16 and codes.shape[1] == d, "d % 16 == 0 and codes [cap, d]")
    if sel is not None:
        _req(row0 == 0, "sel and row0 exclude each other")
        _row_index(sel, "sel", n, cap)
    else:
        _req(0 <= row0 and row0 + n <= cap, "rows [row0, row0 + n) outside codes")
    _check(lib().da_index_dequant_rows(_ptr(codes), _ptr(scale), cap, d, row0, _ptr(sel), n, _ptr(out), _stream()),
           "index_dequant_rows")
    return out


def _filter_args(N, Q, slots, bitmap):
    W = 0
    if slots is not None:
        _i32(slots, "slots")
        _req(slots.numel() >= N, "slots length")
    if bitmap is not None:
        _req(slots is not None, "bitmap needs slots")
        _req(bitmap.dtype == torch.int32 and bitmap.is_contiguous() and bitmap.shape[0] == Q, "bitmap [Q, W] int32")
        W = bitmap.shape[1]
    return W


def topk_dense8(codes, scale, Qv, K: int, thr: float, slots=None, bitmap=None):
    """topk_dense over fp8 rows: exact top-K of Qv @ (codes * scale)^T (fp32 accumulation) per query
    with threshold and optional doc-slot bitmap. d must be one of DENSE8_DIMS: there is no slower fp8
    kernel behind the streaming scan (more than 256 queries run as passes of 256). The partitioning
    is topk_dense's."""
    _bf16_cuda(Qv, "Qv")
    N, d = codes.shape
    Q = Qv.shape[0]
    _codes_cuda(codes, scale, N)
    _req(Qv.dim() == 2 and Qv.is_contiguous() and Qv.shape[1] == d and Qv.data_ptr() % 16 == 0, "Qv layout")
    _req(d in DENSE8_DIMS, f"fp8 dense scan: d must be one of {DENSE8_DIMS}, got {d}")
    _req(1 <= K <= 32 and N > 0, "1 <= K <= 32, N > 0")
    W = _filter_args(N, Q, slots, bitmap)
    if Q > 256:  # the scan's batch limit (topk_dense's streaming path has the same): 256 queries per pass
        parts = [topk_dense8(codes, scale, Qv[a:a + 256], K, thr, slots,
                             None if bitmap is None else bitmap[a:a + 256]) for a in range(0, Q, 256)]
        return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    n4 = (N + 3) // 4 * 4
    if scale.numel() < n4 or scale.data_ptr() % 16:
        # the scan reads the scales of a tile's 4-row groups with one aligned 16-B load
        pad = torch.ones(n4, dtype=torch.float32, device=scale.device)
        pad[:N] = scale[:N]
        scale = pad
    rpw = max(64, math.ceil(N / (256 * 16) / 16) * 16)
    ws = _workspace(int(lib().da_topk_dense_stream8_ws(N, Q, K, rpw)), codes.device)
    out_s = torch.empty((Q, K), dtype=torch.float32, device=codes.device)
    out_i = torch.empty((Q, K), dtype=torch.int32, device=codes.device)
    _check(lib().da_topk_dense_stream8(_ptr(codes), _ptr(scale), N, d, _ptr(slots), _ptr(Qv), Q, _ptr(bitmap), W,
                                       float(thr), K, rpw, _ptr(ws), _ptr(out_s), _ptr(out_i), _stream()),
           "topk_dense_stream8")
    return out_s, out_i


def topk_ranges8(codes, scale, Qv, ranges, range_off, K: int, thr: float, max_rows: int, slots=None, bitmap=None,
                 rows_per_split: int = 512):
    """topk_ranges over fp8 rows. ranges int32 [R, 2] (inside [0, N)), range_off int32 [Q+1]; max_rows =
    max total rows of any query (host int) — sets the split count."""
    _bf16_cuda(Qv, "Qv")
    N, d = codes.shape
    Q = Qv.shape[0]
    _codes_cuda(codes, scale, N)
    _req(Qv.dim() == 2 and Qv.is_contiguous() and Qv.shape[1] == d and Qv.data_ptr() % 16 == 0, "Qv layout")
    _req(d % 16 == 0 and d <= 4096 and 1 <= K <= 32, "d / K limits")
    _i32(ranges, "ranges"); _i32(range_off, "range_off")
    _req(range_off.numel() == Q + 1, "range_off length")
    W = _filter_args(N, Q, slots, bitmap)
    splits = max(1, math.ceil(max_rows / rows_per_split))
    ws = _workspace(splits * Q * K * 8, codes.device)
    out_s = torch.empty((Q, K), dtype=torch.float32, device=codes.device)
    out_i = torch.empty((Q, K), dtype=torch.int32, device=codes.device)
    _check(lib().da_topk_ranges8(_ptr(codes), _ptr(scale), d, _ptr(slots), _ptr(Qv), Q, _ptr(ranges),
                                 _ptr(range_off), _ptr(bitmap), W, float(thr), K, splits, rows_per_split, _ptr(ws),
                                 _ptr(out_s), _ptr(out_i), _stream()), "topk_ranges8")
    return out_s, out_i


def topk_merge(cand_s, cand_i, K: int):
    """cand [P, Q, K] (consumed) -> [Q, K]."""
    _req(cand_s.dtype == torch.float32 and cand_i.dtype == torch.int32, "dtypes")
    P, Q, K2 = cand_s.shape
    _req(K2 == K, "K mismatch")
    cs, ci = cand_s.contiguous().clone(), cand_i.contiguous().clone()
    out_s = torch.empty((Q, K), dtype=torch.float32, device=cs.device)
    out_i = torch.empty((Q, K), dtype=torch.int32, device=cs.device)
    _check(lib().da_topk_merge(_ptr(cs), _ptr(ci), P, Q, K, _ptr(out_s), _ptr(out_i), _stream()), "topk_merge")
    return out_s, out_i


def kmeans_accum(X, assign, sums, counts):
    _bf16_cuda(X, "X"); _i32(assign, "assign")
    N, d = X.shape
    _req(sums.dtype == torch.float32 and sums.shape[1] == d and counts.dtype == torch.float32, "sums/counts fp32")
    _check(lib().da_kmeans_accum(_ptr(X), N, d, _ptr(assign), _ptr(sums), _ptr(counts), _stream()), "kmeans_accum")


def kmeans_accum8(codes, scale, assign, sums, counts):
    """kmeans_accum over fp8 rows: sums[assign[r]] += codes[r] * scale[r] (exact terms), counts[assign[r]]
    += 1 for every row with assign[r] >= 0. Rows with assign < 0 and lists that get no row change nothing."""
    N, d = codes.shape
    _codes_cuda(codes, scale, N)
    _i32(assign, "assign")
    _req(assign.numel() == N, "assign length")
    _req(d % 16 == 0 and d >= 16, "d % 16 == 0")
    _req(sums.is_cuda and sums.dtype == torch.float32 and sums.dim() == 2 and sums.is_contiguous()
         and sums.shape[1] == d, "sums must be contiguous fp32 [L, d] on GPU")
    L = sums.shape[0]
    _req(counts.is_cuda and counts.dtype == torch.float32 and counts.is_contiguous() and counts.numel() == L,
         "counts must be contiguous fp32 [L] on GPU")
    _req(L >= 1, "no lists")
    _check(lib().da_kmeans_accum8(_ptr(codes), _ptr(scale), N, d, _ptr(assign), L, _ptr(sums), _ptr(counts),
                                  _stream()), "kmeans_accum8")


def reserve_workspace(nbytes: int, device=None) -> None:
    """Pre-size the shared split-K / decode workspace. Must be called before capturing HIP graphs
    so the captured kernels keep pointing at a live buffer."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    _workspace(nbytes, dev)


def spin(us: int, device=None) -> None:
    """Hold the current stream busy for ``us`` microseconds (one wave polling the wall clock;
    bounded to 10 s). Test helper: work queued behind it on this stream is provably still pending."""
    _req(0 <= us <= 10_000_000, "spin: 0 <= us <= 1e7")
    _check(lib().da_spin(int(us), None, _stream()), "da_spin")


def gemm8p_persist(on: int = -1) -> int:
    """Persistent tile loop of the prefill GEMM (one workgroup per CU walking its XCD's tiles) on
    (1) / off (0) for later launches; -1 only queries. Returns the previous setting."""
    return int(lib().da_gemm8p_persist(int(on)))


def gemm4w_variant(v: int = -1) -> int:
    """Schedule of the four-wave 256x256 kernel (tile 13, csrc/gemm4w.hip) where K / 64 is even and
    >= 4: 0 = three fragment sets, two barriers per K-tile (default), 1 = two sets, 2 = three sets,
    one barrier; -1 only queries. Returns the previous setting."""
    return int(lib().da_gemm4w_variant(int(v)))


def _f16_cuda(t, name):
    _req(t.is_cuda, f"{name} must be on GPU")
    _req(t.dtype == torch.float16, f"{name} must be fp16, got {t.dtype}")


def gemm_f16(a, w, bias=None, epi: int = EPI_NONE, resid=None, out=None) -> torch.Tensor:
    """out = epi(a @ w^T) in fp16 (fp32 accumulate); epi NONE / BIAS / GELU / RESID."""
    _f16_cuda(a, "a"); _f16_cuda(w, "w")
    M, K = a.shape
    N = w.shape[0]
    _req(w.shape[1] == K and w.is_contiguous() and a.stride(1) == 1 and a.stride(0) % 8 == 0, "gemm_f16 layout")
    _req(K % 64 == 0 and K >= 128 and N % 8 == 0, f"gemm_f16 shape N={N} K={K}")
    _req(epi in (EPI_NONE, EPI_BIAS, EPI_GELU, EPI_RESID), "gemm_f16 epilogue")
    if bias is not None:
        _f16_cuda(bias, "bias"); _req(bias.numel() == N, "bias")
    ldr = 0
    if epi == EPI_RESID:
        _f16_cuda(resid, "resid")
        _req(resid.shape == (M, N) and resid.stride(1) == 1 and resid.stride(0) % 8 == 0, "resid")
        ldr = resid.stride(0)
    if out is None:
        out = torch.empty((M, N), dtype=torch.float16, device=a.device)
    _req(out.dtype == torch.float16 and out.shape == (M, N) and out.stride(1) == 1 and out.stride(0) % 8 == 0, "out")
    _check(lib().da_gemm_f16(_ptr(a), a.stride(0), _ptr(w), _ptr(out), out.stride(0), _ptr(bias), _ptr(resid), ldr,
                             M, N, K, epi, gemm_plan.prefill_bm(M, N, _cus(a.device)), _stream()), "gemm_f16")
    return out


def flash_attn_f16(q, k, v, cu_seqlens, max_seqlen: int, H: int, Hkv: int, D: int, causal: bool = False,
                   scale: float | None = None, out=None):
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        _f16_cuda(t, n)
        _req(t.dim() == 2 and t.stride(1) == 1 and t.stride(0) % 8 == 0 and t.data_ptr() % 16 == 0, f"{n} layout")
    _i32(cu_seqlens, "cu_seqlens")
    _req(D in (64, 96) and H % Hkv == 0, "flash_attn_f16: D 64 / 96")
    T = q.shape[0]
    if out is None:
        out = torch.empty((T, H * D), dtype=torch.float16, device=q.device)
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    _check(lib().da_flash_attn_f16(_ptr(q), _ptr(k), _ptr(v), q.stride(0), k.stride(0), v.stride(0), _ptr(cu_seqlens),
                                   cu_seqlens.numel() - 1, int(max_seqlen), H, Hkv, D, int(causal), float(scale),
                                   _ptr(out), out.stride(0), _stream()), "flash_attn_f16")
    return out


def layernorm_f16(x, g, b, eps: float, resid=None, out=None):
    _f16_cuda(x, "x")
    M, D = x.shape
    _req(x.is_contiguous(), "x must be contiguous")
    _row_d(D, "layernorm_f16")
    if resid is not None:
        _f16_cuda(resid, "resid"); _req(resid.is_contiguous() and resid.shape == x.shape, "bad resid")
    _row_vec(g, D, torch.float16, "g")
    if b is not None:
        _row_vec(b, D, torch.float16, "b")
    if out is None:
        out = torch.empty_like(x)
    _row_out(out, M, D, torch.float16, "out")
    _check(lib().da_layernorm_f16(_ptr(x), _ptr(resid), _ptr(g), _ptr(b), _ptr(out), M, D, float(eps), _stream()),
           "layernorm_f16")
    return out


def bert_embed_ln_f16(ids, positions, types, word, pos, type_, g, b, eps: float, out=None):
    _i32(ids, "ids"); _i32(positions, "positions")
    if types is not None:
        _i32(types, "types")
    _req(word.dim() == 2, "word must be [rows, D]")
    T, D = ids.numel(), word.shape[1]
    _req(positions.numel() == T and (types is None or types.numel() == T), "positions / types length")
    _row_d(D, "bert_embed_ln_f16")
    for t, n in ((word, "word"), (pos, "pos"), (type_, "type")):
        _row_table(t, D, torch.float16, n)
    _row_vec(g, D, torch.float16, "g"); _row_vec(b, D, torch.float16, "b")
    if out is None:
        out = torch.empty((T, D), dtype=torch.float16, device=ids.device)
    _row_out(out, T, D, torch.float16, "out")
    _check(lib().da_bert_embed_ln_f16(_ptr(ids), _ptr(positions), _ptr(types), _ptr(word), _ptr(pos), _ptr(type_),
                                      _ptr(g), _ptr(b), _ptr(out), T, D, float(eps), _stream()), "bert_embed_ln_f16")
    return out


def pool_l2norm_f16(h, cu_seqlens, mode: int = 0, out32=None, out16=None):
    """fp16 hidden states -> unit-norm pooled rows, fp32 and / or bf16 (the index storage type)."""
    _f16_cuda(h, "h"); _i32(cu_seqlens, "cu_seqlens")
    _req(h.dim() == 2 and h.is_contiguous(), "h must be contiguous [T, D]")
    B, D = cu_seqlens.numel() - 1, h.shape[1]
    _row_d(D, "pool_l2norm_f16")
    if out32 is None and out16 is None:
        out32 = torch.empty((B, D), dtype=torch.float32, device=h.device)
    _pool_outs(B, D, out32, out16)
    _check(lib().da_pool_l2norm_f16(_ptr(h), _ptr(cu_seqlens), B, D, mode, _ptr(out32), _ptr(out16), _stream()),
           "pool_l2norm_f16")
    return out32 if out32 is not None else out16
