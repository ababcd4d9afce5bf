"""ISA lint of gemm_dk on fp8 weights (CPU: hipcc cross-compiles gemm_dk_w8.hip to assembly with the
production flags): every instance keeps everything in registers, unpacks the codes with
v_cvt_pk_f32_fp8 and multiplies on the bf16 MFMA (never an fp8 MFMA: the activations are not
quantised), streams the codes with non-temporal 16-B loads, and has no loop that waits for each of
its loads before the next."""
import re

import pytest

from test_isa_lint import _asm, _kernels, _serial_load_loops

PREFIX = "_Z17gemm_dk_w8_kernelILi"
# BM 16 / 32 x BN 16 / 32 / 64 x (none | none + norm | resid | from BN 32: SwiGLU | SwiGLU + norm)
INSTANCES = 2 * (3 + 5 + 5)


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    ks = _kernels(_asm("gemm_dk_w8.hip", tmp_path_factory.mktemp("isa_dk_w8")))
    return {n: v for n, v in ks.items() if n.startswith(PREFIX)}


def test_instance_count(kernels):
    assert len(kernels) == INSTANCES, sorted(kernels)


def test_gemm_dk_w8_isa(kernels):
    assert kernels
    for n, (body, scratch) in kernels.items():
        assert scratch == 0, f"{n}: {scratch} B of scratch"
        assert "v_cvt_pk_f32_fp8" in body, f"{n}: no v_cvt_pk_f32_fp8 (the codes are unpacked in registers)"
        assert "v_mfma_f32_16x16x32_bf16" in body, f"{n}: no bf16 MFMA"
        assert not re.search(r"v_mfma_\S*(fp8|bf8)", body), f"{n}: an fp8 MFMA"
        assert re.search(r"global_load_dwordx4 .* nt", body), f"{n}: no non-temporal 16-B code loads"
        assert not _serial_load_loops(body), f"{n}: a loop waits for each load before the next"
