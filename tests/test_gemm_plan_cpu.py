"""ops/gemm_plan.py against the recorded routing table, without a GPU.

tests/golden/gemm_routes.json was recorded at commit 4b02c16 (the parent of the planner), on an
MI355X (256 CUs, in the file's header), by a throwaway script that called that commit's
kernels.gemm / gemm_dk / gemm_resid_norm with the library's launchers replaced by recorders: each
row holds the call's arguments and what reached the library (entry point, tile, split count,
workspace bytes requested; tile 12, the gemm_dk hand-off's id, for the two gemm_dk launchers, which
take no tile), or "error" where the wrapper raised ValueError. Where Python passed tile = 0, that
commit's da_gemm_route(M, N, K, splits) resolved it on the device. Rows: 25 row counts x the
Phi-3-mini / Llama-3-8B / Llama-3-70B TP=8 / BGE-base products and off-grid shapes, explicit tiles
and split counts, rms, gemm_dk with and without ssq_out, gemm_resid_norm.
"""
import json
import subprocess
import sys
from pathlib import Path

import pytest

from docagents_amd.ops import gemm_plan as P

GOLDEN = json.loads((Path(__file__).parent / "golden" / "gemm_routes.json").read_text())
ENTRY = {"gemv": "da_gemm_bf16", "tile": "da_gemm_bf16", "gemm8p": "da_gemm_bf16", "gemm4w": "da_gemm_bf16",
         "dk": "da_gemm_dk", "dk_splitk": "da_gemm_dk_splitk"}


def _plan(r):
    if r["fn"] == "gemm":
        return P.plan(r["M"], r["N"], r["K"], r["epi"], cus=GOLDEN["cus"], tile=r["tile"], splits=r["splits"],
                      rms=r["rms"])
    if r["fn"] == "gemm_dk":
        return P.plan_dk(r["M"], r["N"], r["K"], r["ssq_out"])
    return P.plan_resid_norm(r["M"], r["N"], r["K"], r["tile"], r["splits"])


def test_golden_routes():
    rows = GOLDEN["rows"]
    assert GOLDEN["cus"] == 256 and len(rows) > 1000
    assert {r["fn"] for r in rows} == {"gemm", "gemm_dk", "gemm_resid_norm"}
    bad = []
    for r in rows:
        try:
            p = _plan(r)
        except ValueError:
            got = "ValueError"
        else:
            entry = "da_gemm_resid_rmsnorm" if r["fn"] == "gemm_resid_norm" else ENTRY[p.family]
            got = (entry, p.tile, p.splits, p.ws_bytes)
        want = r.get("error") or (r["entry"], r["out_tile"], r["out_splits"], r["ws_bytes"])
        if got != want:
            bad.append((r, got))
    assert not bad, f"{len(bad)} of {len(rows)} rows differ, first: {bad[:3]}"


def test_golden_covers_every_family_and_tile():
    fam = {_plan(r).family for r in GOLDEN["rows"] if "error" not in r}
    assert fam == {"gemv", "dk", "dk_splitk", "tile", "gemm8p", "gemm4w"}
    tiles = {r["out_tile"] for r in GOLDEN["rows"] if "error" not in r}
    assert tiles >= {P.TILE_128x128, P.TILE_64x128, P.TILE_32x128, P.TILE_GEMV, P.TILE_8P_256, P.TILE_128x128_PF4,
                     P.TILE_128x64_PF4, P.TILE_8P_128, P.TILE_DK, P.TILE_4W}


def test_a_plan_passed_back_explicitly_is_the_same_plan():
    """gemm(..., tile=p.tile, splits=p.splits) launches what the automatic call launched (gemm_route's
    contract; tile 12 stands for both gemm_dk entry points, whose tile argument the library does not take)."""
    for r in GOLDEN["rows"]:
        if r["fn"] == "gemm" and "error" not in r and not r["rms"]:
            p = _plan(r)
            assert P.plan(r["M"], r["N"], r["K"], r["epi"], cus=GOLDEN["cus"], tile=p.tile, splits=p.splits) == p, r


def test_family_follows_tile():
    for tile, fam in ((4, "gemm8p"), (7, "gemm8p"), (10, "gemm8p"), (13, "gemm4w"), (6, "gemv"), (1, "tile"),
                      (8, "tile")):
        assert P.plan(1000, 3072, 3072, cus=256, tile=tile).family == fam


def test_plan_rejects_what_gemm_rejects():
    with pytest.raises(ValueError):
        P.plan(2, 3072, 3072, cus=256, rms=True)
    with pytest.raises(ValueError):
        P.plan(128, 3072, 3072, cus=256, rms=True)
    with pytest.raises(ValueError):
        P.plan(16, 3072, 3040, cus=256)
    with pytest.raises(ValueError):
        P.plan(16, 3076, 3072, cus=256)
    assert P.plan(1, 3072, 3072, cus=256, rms=True).family == "gemv"


def test_decode_dk_flip_is_not_cached(monkeypatch):
    assert P.plan(16, 3072, 3072, cus=256).family == "dk"
    monkeypatch.setattr(P, "DECODE_DK", False)
    assert P.plan(16, 3072, 3072, cus=256) == P.GemmPlan("tile", P.TILE_32x128, 8, 8 * 16 * 3072 * 4)
    assert not P.dk_fusable(16, 3072, 3072)
    monkeypatch.undo()
    assert P.plan(16, 3072, 3072, cus=256).family == "dk"


def test_cus_changes_the_prefill_row_tile():
    # 2614 x 3072: 132 256-row tiles or 252 128-row ones, one wave each on 256 CUs: the cheaper 128-row tile
    assert P.plan(2614, 3072, 3072, cus=256).tile == P.TILE_8P_128
    assert P.prefill_bm(2614, 3072, 256) == 128 and P.prefill_bm(65536, 3072, 256) == 256
    # 1000 x 3072: 48 / 96 tiles; on 64 CUs the 128-row tiles take two waves (2 * 0.72 > 1)
    assert P.prefill_bm(1000, 3072, 256) == 128 and P.prefill_bm(1000, 3072, 64) == 256


def test_dk_parts_mirrors_the_dk_tile_width():
    # dk_bn (csrc/gemm_dk.hip): 64 columns from 192 tiles of 64, 32 from 192 tiles of 32, else 16
    assert P.dk_parts(3072) == 192 and P.dk_parts(4096) == 256 and P.dk_parts(8192) == 256 and P.dk_parts(12288) == 192
    assert P.dk_parts(6144) == 192 and P.dk_parts(768) == 48
    assert P.dk_parts(3072, 33) == 6 and P.dk_parts(3072, 32) == 192 and P.dk_parts(768, 64) == 48


def test_planner_imports_without_torch():
    # (by file: the ops package's __init__ imports torch for its own helpers)
    code = ("import sys, importlib.util as u; s = u.spec_from_file_location('gemm_plan', %r); "
            "P = u.module_from_spec(s); sys.modules['gemm_plan'] = P; s.loader.exec_module(P); "
            "assert P.plan(64, 3072, 3072, cus=256).family == 'dk_splitk'; " % P.__file__ +
            "assert 'torch' not in sys.modules and 'ctypes' not in sys.modules, sorted(sys.modules)")
    r = subprocess.run([sys.executable, "-c", code], cwd=Path(__file__).parent.parent, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_w8_routes_golden():
    """weight_op / keeps_w8_copy against tests/golden/w8_routes.json, recorded at the parent of these
    two functions by a throwaway script (the file's header says how): per (rows, product, ssq_out) the
    op that commit's LlamaDecoder helpers called on a weight with an fp8 copy in each of the three layer
    bodies, and per (product, fp8-prefill flag) whether its _quantise_weights_fp8 kept the copy."""
    g = json.loads((Path(__file__).parent / "golden" / "w8_routes.json").read_text())
    routes, copies = g["routes"], g["copies"]
    assert len(routes) > 900 and len(copies) > 90
    seen = {r[b] for r in routes for b in ("gemm", "dk", "resid_norm") if b in r}
    assert seen == {"gemm", "gemm_w8", "gemm_tile_w8", "gemm_dk", "gemm_dk_w8", "gemm_dk_splitk_w8", "gemm_resid_norm",
                    "gemm_resid_norm_w8"}
    assert {c["keep"] for c in copies} == {True, False}
    assert {r["M"] for r in routes} == {1, 2, 4, 16, 32, 33, 40, 64, 65, 96, 97, 128, 129, 640}
    bad = []
    for r in routes:
        for body in ("gemm", "dk", "resid_norm"):
            if body in r:
                got = P.weight_op(body, r["M"], r["N"], r["K"], r["epi"], ssq_out=r["ssq_out"])
                if got != r[body]:
                    bad.append((body, r, got))
    assert not bad, f"{len(bad)} routes differ, first: {bad[:3]}"
    bad = [c for c in copies if P.keeps_w8_copy(c["N"], c["K"], c["epi"], prefill_fp8=c["prefill_fp8"]) != c["keep"]]
    assert not bad, f"{len(bad)} of {len(copies)} copy answers differ, first: {bad[:3]}"
    # the row sums of a 40-row O projection of width 256 come from the dk kernel itself (no part per 512 columns)
    assert P.weight_op("dk", 40, 256, 256, P.EPI_RESID, ssq_out=True) == "gemm_dk"
    assert P.weight_op("dk", 40, 256, 256, P.EPI_RESID) == "gemm_dk_splitk_w8"
    with pytest.raises(ValueError):
        P.weight_op("prefill", 640, 3072, 3072)


def test_kernels_reexports_the_planners_objects():
    from docagents_amd.ops import kernels as K
    from docagents_amd.ops import reference as R
    for name in ("gemv_fusable", "gemv_w8_fusable", "dk_fusable", "dk_parts"):
        assert getattr(K, name) is getattr(P, name)
    for name in ("gemv_fusable", "gemv_w8_fusable", "dk_fusable", "dk_parts", "dk_w8_fusable", "tile_w8_fusable",
                 "prefill_w8_fusable", "weight_op", "keeps_w8_copy"):
        assert getattr(R, name) is getattr(P, name) and getattr(K, name) is getattr(P, name)
    assert (R.DK_MAX_M, R.DK_SPLITK_ABOVE) == (P.DK_MAX_M, P.DK_SPLITK_ABOVE)
    assert not hasattr(R, "DECODE_DK")  # one switch, the planner's: a copy here would go stale
    assert (K.DK_MAX_M, K.DK_SPLITK_ABOVE) == (P.DK_MAX_M, P.DK_SPLITK_ABOVE) == (64, 32)
    assert not any(hasattr(K, n) for n in ("_auto_splits", "_decode_tile", "_dk_splits", "_dk_splitk"))
    assert "da_gemm_route" not in K._SIGS
