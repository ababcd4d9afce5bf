"""R / U / KS / LW sweep of the MXFP4 GEMV (csrc/gemv_w4.hip) on the five Phi-3-mini batch-1 products:
rows per wave, loads in flight per row and round, waves per row, code bytes per lane and load (8: one
1024-element k-block per wave instruction; 16: two, the odd tail's upper half-wave clamped and
zeroed). The kernel library carries only the winners (launch_gemv_w4); this script compiles the same
source with -DDA_GEMV_W4_SWEEP into a library of its own (bench/_w4_sweep.so; --build, no GPU needed)
that exposes every arm, and times them with bench/w8_decode.py's method (cold weight pool, one
captured graph per arm, interleaved rounds). One JSON line per shape; "lib" is the arm the kernel
library dispatches (da_gemv_w4)."""
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
from w4_decode import product_bytes  # noqa: E402
from w8_decode import EPS, POOL_BYTES, SHAPES, graph_of, pool, shape_operands, time_graphs  # noqa: E402

LIB = os.path.join(HERE, "_w4_sweep.so")


def build():
    cmd = [_hipcc(), *_flags(False), "-DDA_GEMV_W4_SWEEP", "-shared", str(CSRC / "gemv_w4.hip"), "-o", LIB]
    subprocess.run(cmd, check=True)
    return LIB


def arms(N, Kd, epi):
    out = []
    for lw in (8, 16):
        nld = -(-Kd // (lw * 128))  # loads that cover a row
        if epi == K.EPI_SWIGLU:
            out += [(4, u, 1, lw) for u in (1, 2, 3, 4) if u <= nld]
            continue
        for ks in (1, 2):
            if nld < 2 * ks and ks == 2:
                continue
            for r in (1, 2, 4):
                for u in (1, 2, 3, 4):
                    # skip: more loads per round than the wave owns; the largest register arms
                    if u > -(-nld // ks) or r * u * lw > 128:
                        continue
                    out.append((r, u, ks, lw))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", action="store_true", help="compile bench/_w4_sweep.so and exit")
    ap.add_argument("--rounds", type=int, default=6)
    a = ap.parse_args()
    if a.build:
        print(build())
        return
    if not torch.cuda.is_available():
        raise SystemExit("w4_sweep.py measures on the GPU; none found")
    L = ctypes.CDLL(LIB)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.da_gemv_w4_sweep.argtypes = [vp] * 6 + [ci, ci, ci, vp, ctypes.c_float, ci, ci, ci, ci, vp]
    L.da_gemv_w4_sweep.restype = ci
    dev = torch.device("cuda", 0)
    for name, N, Kd, epi, fused in SHAPES:
        w, _, _, x, resid, out = shape_operands(N, Kd, epi, dev)
        q, e = K.quant_weight_mxfp4(w)
        n4 = max(2, POOL_BYTES // (N * Kd // 2))
        w4, e4 = pool(q, n4), pool(e, n4)
        rms = (None, EPS) if fused else None
        want = K.gemm_w4(x, q, e, epi=epi, resid=resid, rms=rms).float()

        def sweep_launch(r, u, ks, lw):
            def launch(i):
                rc = L.da_gemv_w4_sweep(K._ptr(x), K._ptr(w4[i]), K._ptr(e4[i]), K._ptr(out), None, K._ptr(resid), N, Kd,
                                        epi, None, EPS if fused else 0.0, r, u, ks, lw, K._stream())
                if rc:
                    raise RuntimeError(f"da_gemv_w4_sweep R={r} U={u} KS={ks} LW={lw}: hipError {rc}")
            return launch

        graphs = {"lib": graph_of(lambda i: K.gemm_w4(x, w4[i], e4[i], epi=epi, resid=resid, out=out, rms=rms), n4)}
        for r, u, ks, lw in arms(N, Kd, epi):
            graphs[f"R{r}_U{u}_KS{ks}_LW{lw}"] = graph_of(sweep_launch(r, u, ks, lw), n4)
            torch.cuda.synchronize()
            err = float((out.float() - want).abs().max())  # every arm computes the library's result
            assert err <= 0.03 + 0.02 * float(want.abs().max()), (name, r, u, ks, lw, err)
        t = time_graphs(graphs, {k: n4 for k in graphs}, a.rounds)
        nbytes = product_bytes(N, Kd, epi, "mxfp4")
        table = {k: {"us": round(m, 2), "us_min": round(mn, 2), "TBps": round(nbytes / m / 1e6, 2)}
                 for k, (m, mn) in sorted(t.items(), key=lambda kv: kv[1][0])}
        print(json.dumps({"shape": name, "N": N, "K": Kd, "copies": n4, "arms": table}), flush=True)
        del graphs, w4, e4
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
