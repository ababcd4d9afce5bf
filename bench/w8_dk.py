"""fp8 (e4m3) decoder weights vs bf16 at 2..32 rows, one process, arms interleaved (the method of
bench/w8_decode.py: a 1 GiB pool of weight copies per arm so every launch streams cold weights, one
captured graph per pass, median of the rounds; run the command twice, the two runs are the spread):
(a) the five Phi-3-mini products of the gemm_dk decode step at M = 4, 16, 32, as the step runs them
    (QKV / LM head / gate-up with the deferred norm, O / down with residual + row sums of squares):
    kernels.gemm_dk on the dequantised bf16 weights vs kernels.gemm_dk_w8; us per launch.
(b) --sweep: every tile-width / PF arm of csrc/gemm_dk_w8.hip per shape, from a library of its own
    (bench/_w8_dk_sweep.so; --build-sweep compiles it with -DDA_GEMM_DK_W8_SWEEP, no GPU needed);
    "lib" is the arm the kernel library dispatches.
(c) the graph-replayed Phi-3-mini decode step (real dims, random weights, 512 cached tokens per row)
    at batch 4, 16 and 32: LlamaDecoder(weight_dtype="fp8") vs a bf16 decoder on a deep copy of the
    dequantised weights; ms per step. --skip-model: (a) / (b) only.
One JSON line per table."""
import argparse
import copy
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from docagents_amd.ops import kernels as K  # noqa: E402
from docagents_amd.ops.build import CSRC, _flags, _hipcc  # noqa: E402
from w8_decode import POOL_BYTES, graph_of, pool, time_graphs  # noqa: E402

EPS = 1e-5
ROWS = (4, 16, 32)
# name, N, K, epilogue, deferred norm on the input (as LlamaDecoder._decode_step_dk runs them)
SHAPES = [("qkv", 9216, 3072, K.EPI_NONE, True), ("o", 3072, 3072, K.EPI_RESID, False),
          ("gate_up", 16384, 3072, K.EPI_SWIGLU, True), ("down", 3072, 8192, K.EPI_RESID, False),
          ("lm_head", 32064, 3072, K.EPI_NONE, True)]
SWEEP_LIB = os.path.join(HERE, "_w8_dk_sweep.so")
SWEEP_ARMS = [(bn, pf) for bn in (16, 32, 64) for pf in (1, 2, 4, 8)]


def build_sweep():
    cmd = [_hipcc(), *_flags(False), "-DDA_GEMM_DK_W8_SWEEP", "-shared", str(CSRC / "gemm_dk_w8.hip"), "-o", SWEEP_LIB]
    subprocess.run(cmd, check=True)
    return SWEEP_LIB


def operands(M, N, Kd, epi, norm, dev):
    g = torch.Generator(device=dev).manual_seed(N + Kd + M)
    w = (torch.randn(N, Kd, device=dev, generator=g) * Kd ** -0.5).to(torch.bfloat16)
    q, s = K.quant_weight_fp8_pow2(w)
    dq = (q.float() * s[:, None]).to(torch.bfloat16)
    x = torch.randn(M, Kd, device=dev, generator=g).to(torch.bfloat16)
    resid = torch.randn(M, N, device=dev, generator=g).to(torch.bfloat16) if epi == K.EPI_RESID else None
    out = torch.empty((M, N // 2 if epi == K.EPI_SWIGLU else N), dtype=torch.bfloat16, device=dev)
    ssq_out = torch.zeros(512 * 64, dtype=torch.float32, device=dev) if epi == K.EPI_RESID else None
    norm_in = None
    if norm:  # one part holding the rows' sums of squares: the kernels only sum the parts they are told
        ssq = torch.zeros(512 * 64, dtype=torch.float32, device=dev)
        ssq.view(-1, 64)[0, :M] = x.float().pow(2).sum(-1)
        norm_in = (ssq, 192, EPS)  # the part count a Phi-3 step passes (hidden 3072: 192 tiles of 16)
    return dq, q, s, x, dict(epi=epi, resid=resid, out=out, ssq_out=ssq_out, norm_in=norm_in)


def product_arms(dev, rounds, sweep):
    L = None
    if sweep:
        L = ctypes.CDLL(SWEEP_LIB)
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.da_gemm_dk_w8_sweep.argtypes = [vp, ci, vp, vp, vp, ci, vp, vp, ci, ci, ci, ci, ci, vp, ci, ci,
                                          ctypes.c_float, vp, ci, ci, vp]
        L.da_gemm_dk_w8_sweep.restype = ci
    for name, N, Kd, epi, norm in SHAPES:
        for M in ROWS:
            dq, q, s, x, kw = operands(M, N, Kd, epi, norm, dev)
            nb, n8 = max(2, POOL_BYTES // (N * Kd * 2)), max(2, POOL_BYTES // (N * Kd))
            wb, w8 = pool(dq, nb), pool(q, n8)
            want = K.gemm_dk_w8(x, q, s, **{**kw, "out": None}).float()
            graphs = {"bf16": graph_of(lambda i: K.gemm_dk(x, wb[i], **kw), nb),
                      "fp8": graph_of(lambda i: K.gemm_dk_w8(x, w8[i], s, **kw), n8)}
            n = {"bf16": nb, "fp8": n8}
            if sweep:
                ssq, parts, eps = kw["norm_in"] or (None, 0, 0.0)
                out, resid = kw["out"], kw["resid"]

                def arm(bn, pf):
                    def launch(i):
                        rc = L.da_gemm_dk_w8_sweep(K._ptr(x), x.stride(0), K._ptr(w8[i]), K._ptr(s), K._ptr(out),
                                                   out.stride(0), None, K._ptr(resid), N if resid is not None else 0,
                                                   M, N, Kd, epi, K._ptr(ssq), parts, Kd, eps, K._ptr(kw["ssq_out"]),
                                                   bn, pf, K._stream())
                        if rc:
                            raise RuntimeError(f"da_gemm_dk_w8_sweep BN={bn} PF={pf}: hipError {rc}")
                    return launch
                bm = 16 if M <= 16 else 32
                for bn, pf in SWEEP_ARMS:
                    if (epi == K.EPI_SWIGLU and bn < 32) or (pf == 8 and 8 * (bn // 16 + bm // 8) > 48):
                        continue
                    if -(-N // bn) > 512 and epi == K.EPI_RESID:
                        continue
                    key = f"BN{bn}_PF{pf}"
                    graphs[key] = graph_of(arm(bn, pf), n8)
                    n[key] = n8
                    torch.cuda.synchronize()
                    assert torch.equal(out.float(), want), (name, M, bn, pf)  # every arm: the library's bits
            t = time_graphs(graphs, n, rounds)
            row = {"shape": name, "M": M, "N": N, "K": Kd,
                   "us": {k: round(v[0], 2) for k, v in sorted(t.items(), key=lambda kv: kv[1][0])},
                   "us_min": {k: round(v[1], 2) for k, v in t.items()},
                   "fp8_over_bf16": round(t["fp8"][0] / t["bf16"][0], 3)}
            print(json.dumps(row), flush=True)
            del graphs, wb, w8
            torch.cuda.empty_cache()


def step_graph(m, B, ctx):
    """(state, graph, reset) of one captured decode step over B rows with ctx cached tokens each."""
    from docagents_amd.models.llama import DecodeState
    st = DecodeState(m, B, 64, 0.2, 3)
    st.slot.copy_(torch.arange(B, dtype=torch.int32))
    st.tokens.copy_(torch.arange(300, 300 + B, dtype=torch.int32))

    def reset():
        st.pos.fill_(ctx); st.lens.fill_(ctx + 1); st.active.fill_(1); st.start.fill_(ctx); st.hist.fill_(-1)
    reset()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            m.decode_step(st)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        m.decode_step(st)
    return st, g, reset


def model_arms(dev, rounds, steps=16, ctx=512):
    from docagents_amd.models.configs import decoder_config
    from docagents_amd.models.llama import LlamaDecoder
    cfg = decoder_config("phi3-mini")
    f = LlamaDecoder(cfg, dev, seed=0, weight_dtype="fp8")
    strip = lambda d: {k: v for k, v in d.items() if not k.endswith(("_q8", "_s8")) and k != "layers"}  # noqa: E731
    wb = copy.deepcopy({**strip(f.w), "layers": [strip(L) for L in f.w["layers"]]})
    b = LlamaDecoder(cfg, dev, weights=wb)
    for m in (f, b):
        m.alloc_cache(max(ROWS), 1024)
    for B in ROWS:
        arms = {"bf16": step_graph(b, B, ctx), "fp8": step_graph(f, B, ctx)}
        ms = {k: [] for k in arms}
        for rnd in range(rounds + 1):
            for k, (st, g, reset) in arms.items():
                reset()
                a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(steps):
                    g.replay()
                e.record()
                torch.cuda.synchronize()
                if rnd > 0:
                    ms[k].append(a.elapsed_time(e) / steps)
        row = {"phi3_mini_step": True, "B": B, "ctx": ctx,
               "ms_per_step": {k: round(float(np.median(v)), 4) for k, v in ms.items()},
               "ms_per_step_min": {k: round(float(np.min(v)), 4) for k, v in ms.items()}}
        row["fp8_over_bf16"] = round(row["ms_per_step"]["fp8"] / row["ms_per_step"]["bf16"], 3)
        print(json.dumps(row), flush=True)
        del arms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-sweep", action="store_true", help="compile bench/_w8_dk_sweep.so and exit")
    ap.add_argument("--sweep", action="store_true", help="add the tile-width / PF arms of the sweep library")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--skip-products", action="store_true")
    a = ap.parse_args()
    if a.build_sweep:
        print(build_sweep())
        return
    if not torch.cuda.is_available():
        raise SystemExit("w8_dk.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    if not a.skip_products:
        product_arms(dev, a.rounds, a.sweep)
    if not a.skip_model:
        model_arms(dev, a.rounds)


if __name__ == "__main__":
    main()
