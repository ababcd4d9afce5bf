"""ISA lint of the fp8 index scans (CPU: hipcc cross-compiles vecsearch8.hip to assembly with the
production flags): every instance of the streaming scan, the shared-tile scan and the ranges scan
keeps everything in registers, unpacks the codes with v_cvt_pk_f32_fp8 (no fp8 MFMA: the query is
not quantised), and has no loop that waits for each of its loads before the next."""
import re

import pytest

from test_isa_lint import _asm, _kernels, _serial_load_loops

SCANS = {"_Z25topk_dense_stream8_kernelILi": 4, "_Z21topk_dense_mq8_kernelILi": 4, "_Z19topk_ranges8_kernel": 1}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return _kernels(_asm("vecsearch8.hip", tmp_path_factory.mktemp("isa8")))


@pytest.mark.parametrize("prefix", sorted(SCANS))
def test_fp8_scans_isa(kernels, prefix):
    hits = {n: v for n, v in kernels.items() if n.startswith(prefix)}
    assert len(hits) == SCANS[prefix], f"{prefix}*: expected {SCANS[prefix]} instances (d = 128, 384, 768, 1024), " \
                                       f"got {sorted(hits)}"
    for n, (body, scratch) in hits.items():
        assert scratch == 0, f"{n}: {scratch} B of scratch"
        assert "v_cvt_pk_f32_fp8" in body, f"{n}: no v_cvt_pk_f32_fp8 (the codes are unpacked in registers)"
        assert not _serial_load_loops(body), f"{n}: a loop waits for each load before the next"
        # bf16 MFMA on the unpacked codes; never an fp8 x fp8 MFMA
        assert not re.search(r"v_mfma_\S*(fp8|bf8)", body), f"{n}: an fp8 MFMA"
        if "dense" in n:
            assert "v_mfma_f32_16x16x32_bf16" in body, n


def test_fp8_dense_scans_stream_rows_non_temporally(kernels):
    """The dense scans read the codes with non-temporal 16-B loads, as the bf16 scans read their rows."""
    for n, (body, _) in kernels.items():
        if not (n.startswith("_Z25topk_dense_stream8_kernelILi") or n.startswith("_Z21topk_dense_mq8_kernelILi")):
            continue
        assert re.search(r"global_load_dwordx4 .* nt", body), f"{n}: no non-temporal 16-B row loads"
