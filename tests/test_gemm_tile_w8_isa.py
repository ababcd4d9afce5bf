"""ISA lint of the fp8-weight decode tiles (csrc/gemm_tile_w8.hip), cross-compiled on the CPU: every
instance unpacks the codes with v_cvt_pk_f32_fp8, multiplies on the bf16 MFMA (never an fp8 / bf8 one:
the activations are not quantised), keeps its prefetch ring in registers (no scratch) and has no
loop that waits for each load before the next."""
import re

from test_isa_lint import _asm, _kernels, _serial_load_loops

PREFIX = "_Z19gemm_tile_w8_kernel"
# 2 tiles (64x128, 128x64) x 5 epilogues (NONE, BIAS, SWIGLU, RESID, PARTIAL) x non-temporal loads off / on
INSTANCES = 2 * 5 * 2


def test_gemm_tile_w8_kernels_isa(tmp_path):
    ks = {n: v for n, v in _kernels(_asm("gemm_tile_w8.hip", tmp_path)).items() if n.startswith(PREFIX)}
    assert len(ks) == INSTANCES, sorted(ks)
    for n, (body, scratch) in ks.items():
        assert scratch == 0, f"{n}: {scratch} B of scratch"
        assert "v_cvt_pk_f32_fp8" in body, f"{n}: no v_cvt_pk_f32_fp8"
        assert "v_mfma_f32_16x16x32_bf16" in body, f"{n}: no bf16 MFMA"
        assert not re.search(r"v_mfma\w*(fp8|bf8)", body), f"{n}: an fp8 / bf8 MFMA"
        assert not _serial_load_loops(body), f"{n}: a loop waits for each load before the next"
