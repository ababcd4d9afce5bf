"""R / U / KS sweep of the fp8 GEMV (csrc/gemv_w8.hip) on the five Phi-3-mini batch-1 products: rows
per wave, k-blocks in flight per round, waves per row. The kernel library carries only the winners
(launch_gemv_w8); this script compiles the same source with -DDA_GEMV_W8_SWEEP into a library of
its own (bench/_w8_sweep.so; --build, no GPU needed) that exposes every arm, and times them with
bench/w8_decode.py's method (cold weight pool, one captured graph per arm, interleaved rounds).
One JSON line per shape; "lib" is the arm the kernel library dispatches (da_gemv_w8)."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from docagents_amd.ops import kernels as K  # noqa: E402
from docagents_amd.ops.build import CSRC, _flags, _hipcc  # noqa: E402
from w8_decode import EPS, POOL_BYTES, SHAPES, graph_of, pool, product_bytes, shape_operands, time_graphs  # noqa: E402

LIB = os.path.join(HERE, "_w8_sweep.so")


def build():
    cmd = [_hipcc(), *_flags(False), "-DDA_GEMV_W8_SWEEP", "-shared", str(CSRC / "gemv_w8.hip"), "-o", LIB]
    subprocess.run(cmd, check=True)
    return LIB


def arms(N, Kd, epi):
    nkb = Kd // 1024
    if epi == K.EPI_SWIGLU:
        return [(4, u, 1) for u in (1, 2, 3, 4) if u <= nkb]
    out = []
    for ks in (1, 2):
        if nkb % ks:
            continue
        for r in (1, 2, 4, 8):
            for u in (1, 2, 3, 4, 8):
                # skip: more blocks per round than the wave owns, 256-VGPR arms (1 wave / SIMD)
                if u > nkb // ks or (ks == 2 and r == 8) or r * u > 16:
                    continue
                out.append((r, u, ks))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", action="store_true", help="compile bench/_w8_sweep.so and exit")
    ap.add_argument("--rounds", type=int, default=6)
    a = ap.parse_args()
    if a.build:
        print(build())
        return
    if not torch.cuda.is_available():
        raise SystemExit("w8_sweep.py measures on the GPU; none found")
    L = ctypes.CDLL(LIB)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.da_gemv_w8_sweep.argtypes = [vp] * 6 + [ci, ci, ci, vp, ctypes.c_float, ci, ci, ci, vp]
    L.da_gemv_w8_sweep.restype = ci
    dev = torch.device("cuda", 0)
    for name, N, Kd, epi, fused in SHAPES:
        w, q, s, x, resid, out = shape_operands(N, Kd, epi, dev)
        n8 = max(2, POOL_BYTES // (N * Kd))
        w8 = pool(q, n8)
        rms = (None, EPS) if fused else None
        want = K.gemm_w8(x, q, s, epi=epi, resid=resid, rms=rms).float()

        def sweep_launch(r, u, ks):
            def launch(i):
                rc = L.da_gemv_w8_sweep(K._ptr(x), K._ptr(w8[i]), K._ptr(s), K._ptr(out), None, K._ptr(resid), N, Kd,
                                        epi, None, EPS if fused else 0.0, r, u, ks, K._stream())
                if rc:
                    raise RuntimeError(f"da_gemv_w8_sweep R={r} U={u} KS={ks}: hipError {rc}")
            return launch

        graphs = {"lib": graph_of(lambda i: K.gemm_w8(x, w8[i], s, epi=epi, resid=resid, out=out, rms=rms), n8)}
        for r, u, ks in arms(N, Kd, epi):
            graphs[f"R{r}_U{u}_KS{ks}"] = graph_of(sweep_launch(r, u, ks), n8)
            torch.cuda.synchronize()
            err = float((out.float() - want).abs().max())  # every arm computes the library's result
            assert err <= 0.03 + 0.02 * float(want.abs().max()), (name, r, u, ks, err)
        t = time_graphs(graphs, {k: n8 for k in graphs}, a.rounds)
        nbytes = product_bytes(N, Kd, epi, 1)
        table = {k: {"us": round(m, 2), "us_min": round(mn, 2), "TBps": round(nbytes / m / 1e6, 2)}
                 for k, (m, mn) in sorted(t.items(), key=lambda kv: kv[1][0])}
        print(json.dumps({"shape": name, "N": N, "K": Kd, "copies": n8, "arms": table}), flush=True)
        del graphs, w8
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
