"""fp8 (e4m3) decoder weights vs bf16 at batch 1, one process, arms interleaved:
(a) the five Phi-3-mini weight-streaming products, bf16 GEMV (kernels.gemm) vs fp8 GEMV
    (kernels.gemm_w8), with the fused RMSNorm where the model fuses it. Every launch streams a
    different copy of the matrix (a pool larger than the 256 MB Infinity Cache, as a decode step
    streams every weight once) and the launches of one pass replay from one captured graph (as the
    decode graph issues them); us per launch and TB/s from the bytes the shapes imply.
(b) Phi-3-mini (real dims, random weights) Generator.generate of one 2.9k-token prompt, 64 new
    tokens, LlamaDecoder(weight_dtype="bf16") vs ("fp8"): ms per answer and decode ms per step.
One JSON line. --skip-model: (a) only."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from docagents_amd.ops import kernels as K  # noqa: E402

EPS = 1e-5
# name, N, K, epilogue, RMSNorm fused (as LlamaDecoder's batch-1 step runs them)
SHAPES = [("qkv", 9216, 3072, K.EPI_NONE, True), ("o", 3072, 3072, K.EPI_RESID, False),
          ("gate_up", 16384, 3072, K.EPI_SWIGLU, True), ("down", 3072, 8192, K.EPI_RESID, False),
          ("lm_head", 32064, 3072, K.EPI_NONE, True)]
POOL_BYTES = 1 << 30  # distinct weight bytes per arm and pass: 4x the Infinity Cache


def product_bytes(N, Kd, epi, wbytes):
    """Bytes one launch has to move: the weights, their row scales (fp8), the activation row, the
    residual row and the output row."""
    nout = N // 2 if epi == K.EPI_SWIGLU else N
    return N * Kd * wbytes + (N * 4 if wbytes == 1 else 0) + Kd * 2 + nout * 2 + (N * 2 if epi == K.EPI_RESID else 0)


def pool(w, copies):
    return [w.clone() for _ in range(copies)]


def graph_of(launch, n):
    """One captured graph of launch(0) .. launch(n - 1) on a side stream (warmed first)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for i in range(n):
            launch(i)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(n):
            launch(i)
    return g


def time_graphs(graphs: dict, launches: dict, rounds: int):
    """Interleaved rounds of the arms' graphs; us per launch (median and min over the rounds)."""
    ev = {k: [] for k in graphs}
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, g in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); g.replay(); b.record()
            ev[k].append((a, b))
    torch.cuda.synchronize()
    out = {}
    for k, pairs in ev.items():
        us = np.array([a.elapsed_time(b) * 1e3 / launches[k] for a, b in pairs])
        out[k] = (float(np.median(us)), float(us.min()))
    return out


def shape_operands(N, Kd, epi, dev):
    g = torch.Generator(device=dev).manual_seed(N + Kd)
    w = (torch.randn(N, Kd, device=dev, generator=g) * Kd ** -0.5).to(torch.bfloat16)
    q, s = K.quant_weight_fp8_pow2(w)
    x = (torch.randn(1, Kd, device=dev, generator=g)).to(torch.bfloat16)
    resid = torch.randn(1, N, device=dev, generator=g).to(torch.bfloat16) if epi == K.EPI_RESID else None
    out = torch.empty((1, N // 2 if epi == K.EPI_SWIGLU else N), dtype=torch.bfloat16, device=dev)
    return w, q, s, x, resid, out


def gemv_arms(dev, rounds):
    res = {}
    for name, N, Kd, epi, fused in SHAPES:
        w, q, s, x, resid, out = shape_operands(N, Kd, epi, dev)
        rms = (None, EPS) if fused else None
        nb, n8 = max(2, POOL_BYTES // (N * Kd * 2)), max(2, POOL_BYTES // (N * Kd))
        wb, w8 = pool(w, nb), pool(q, n8)
        graphs = {
            "bf16": graph_of(lambda i: K.gemm(x, wb[i], epi=epi, resid=resid, out=out, rms=rms), nb),
            "fp8": graph_of(lambda i: K.gemm_w8(x, w8[i], s, epi=epi, resid=resid, out=out, rms=rms), n8),
        }
        t = time_graphs(graphs, {"bf16": nb, "fp8": n8}, rounds)
        r = {"N": N, "K": Kd}
        for arm, wbytes in (("bf16", 2), ("fp8", 1)):
            med, mn = t[arm]
            r[arm] = {"us": round(med, 2), "us_min": round(mn, 2),
                      "TBps": round(product_bytes(N, Kd, epi, wbytes) / med / 1e6, 2)}
        r["fp8_over_bf16"] = round(t["fp8"][0] / t["bf16"][0], 3)
        res[name] = r
        del graphs, wb, w8
        torch.cuda.empty_cache()
    return res


def model_arms(dev, rounds):
    from docagents_amd.engine.generator import Generator
    from docagents_amd.models.configs import decoder_config
    from docagents_amd.models.llama import LlamaDecoder
    cfg = decoder_config("phi3-mini")
    prompt = np.random.default_rng(0).integers(300, cfg.vocab, size=2900).tolist()
    gens = {}
    for arm in ("bf16", "fp8"):
        m = LlamaDecoder(cfg, dev, seed=0, weight_dtype=arm)
        m.alloc_cache(4, 4096)
        gens[arm] = Generator(m, max_batch=1, max_seq=4096, temperature=0.2, seed=3, eos=())
    ms = {k: [] for k in gens}
    step_ms = {k: [] for k in gens}
    for rnd in range(rounds + 1):
        for arm, g in gens.items():
            d0, n0 = g.stats["decode_s"], g.stats["decode_steps"]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = g.generate([prompt], 64)
            torch.cuda.synchronize()
            if rnd > 0:  # round 0 captures the graphs
                ms[arm].append((time.perf_counter() - t0) * 1e3)
                step_ms[arm].append((g.stats["decode_s"] - d0) * 1e3 / max(1, g.stats["decode_steps"] - n0))
            assert len(out[0].tokens) == 64
    return {arm: {"ms_per_answer": round(float(np.median(ms[arm])), 2),
                  "ms_per_answer_min": round(float(np.min(ms[arm])), 2),
                  "decode_ms_per_step": round(float(np.median(step_ms[arm])), 4)} for arm in gens}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--model-rounds", type=int, default=5)
    ap.add_argument("--skip-model", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("w8_decode.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    res = {"bench": "w8_decode", "gemv": gemv_arms(dev, a.rounds)}
    if not a.skip_model:
        res["phi3_mini_b1"] = model_arms(dev, a.model_rounds)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
