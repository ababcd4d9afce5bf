"""ISA lint of the batch-1 GEMV on MXFP4 weights (CPU: hipcc cross-compiles gemv_w4.hip to assembly
with the production flags): every instance keeps everything in registers, unpacks the codes with
v_cvt_scalef32_pk_f32_fp4 (the block scale is the instruction's own operand), streams the codes with
non-temporal vector loads, multiplies on the VALU (a one-row product has nothing for an MFMA), and
has no loop that waits for each of its loads before the next."""
import re

import pytest

from test_isa_lint import _asm, _kernels, _serial_load_loops

PREFIX = "_Z14gemv_w4_kernelILi"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    ks = _kernels(_asm("gemv_w4.hip", tmp_path_factory.mktemp("isa_gemv_w4")))
    return {n: v for n, v in ks.items() if n.startswith(PREFIX)}


def test_gemv_w4_isa(kernels):
    assert len(kernels) >= 5, sorted(kernels)  # at least one instance per Phi-3-mini product
    for n, (body, scratch) in kernels.items():
        assert scratch == 0, f"{n}: {scratch} B of scratch"
        assert "v_cvt_scalef32_pk_f32_fp4" in body, f"{n}: no v_cvt_scalef32_pk_f32_fp4 (the codes are unpacked in registers)"
        assert re.search(r"global_load_dwordx[24] .* nt", body), f"{n}: no non-temporal vector code loads"
        assert not _serial_load_loops(body), f"{n}: a loop waits for each load before the next"
        assert "v_mfma" not in body, f"{n}: an MFMA in a one-row product"
