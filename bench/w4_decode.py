"""MXFP4 decoder weights vs fp8 (e4m3) and bf16 at batch 1, one process, arms interleaved, with the
method of bench/w8_decode.py (whose helpers this imports):
(a) the five Phi-3-mini weight-streaming products, bf16 GEMV (kernels.gemm) vs fp8 GEMV
    (kernels.gemm_w8) vs MXFP4 GEMV (kernels.gemm_w4), with the fused RMSNorm where the model fuses
    it. Every launch streams a different copy of the matrix (a pool larger than the 256 MB Infinity
    Cache) and the launches of one pass replay from one captured graph; us per launch and TB/s from
    the bytes the shapes imply.
(b) Phi-3-mini (real dims, random weights) Generator.generate of one 2.9k-token prompt, 64 new
    tokens, LlamaDecoder(weight_dtype=...) for bf16 / fp8 / mxfp4: ms per answer, decode ms per step.
One JSON line. --skip-model: (a) only. Run it twice: the spread of the two runs is the noise floor."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from docagents_amd.ops import kernels as K  # noqa: E402
from w8_decode import EPS, POOL_BYTES, SHAPES, graph_of, pool, shape_operands, time_graphs  # noqa: E402

WBYTES = {"bf16": 2.0, "fp8": 1.0, "mxfp4": 0.53125}


def product_bytes(N, Kd, epi, arm):
    """Bytes one launch has to move: the weights with their scales (fp8: fp32 per row, in WBYTES for
    mxfp4), the activation row, the residual row and the output row."""
    nout = N // 2 if epi == K.EPI_SWIGLU else N
    return (int(N * Kd * WBYTES[arm]) + (N * 4 if arm == "fp8" else 0) + Kd * 2 + nout * 2
            + (N * 2 if epi == K.EPI_RESID else 0))


def gemv_arms(dev, rounds):
    res = {}
    for name, N, Kd, epi, fused in SHAPES:
        w, q8, s8, x, resid, out = shape_operands(N, Kd, epi, dev)
        q4, e4 = K.quant_weight_mxfp4(w)
        rms = (None, EPS) if fused else None
        n = {"bf16": max(2, POOL_BYTES // (N * Kd * 2)), "fp8": max(2, POOL_BYTES // (N * Kd)),
             "mxfp4": max(2, POOL_BYTES // (N * Kd // 2))}
        wb, w8, w4, s4 = pool(w, n["bf16"]), pool(q8, n["fp8"]), pool(q4, n["mxfp4"]), pool(e4, n["mxfp4"])
        graphs = {
            "bf16": graph_of(lambda i: K.gemm(x, wb[i], epi=epi, resid=resid, out=out, rms=rms), n["bf16"]),
            "fp8": graph_of(lambda i: K.gemm_w8(x, w8[i], s8, epi=epi, resid=resid, out=out, rms=rms), n["fp8"]),
            "mxfp4": graph_of(lambda i: K.gemm_w4(x, w4[i], s4[i], epi=epi, resid=resid, out=out, rms=rms), n["mxfp4"]),
        }
        t = time_graphs(graphs, n, rounds)
        r = {"N": N, "K": Kd}
        for arm in graphs:
            med, mn = t[arm]
            r[arm] = {"us": round(med, 2), "us_min": round(mn, 2),
                      "TBps": round(product_bytes(N, Kd, epi, arm) / med / 1e6, 2)}
        r["mxfp4_over_bf16"] = round(t["mxfp4"][0] / t["bf16"][0], 3)
        r["mxfp4_over_fp8"] = round(t["mxfp4"][0] / t["fp8"][0], 3)
        res[name] = r
        del graphs, wb, w8, w4, s4
        torch.cuda.empty_cache()
    return res


def model_arms(dev, rounds):
    from docagents_amd.engine.generator import Generator
    from docagents_amd.models.configs import decoder_config
    from docagents_amd.models.llama import LlamaDecoder
    cfg = decoder_config("phi3-mini")
    prompt = np.random.default_rng(0).integers(300, cfg.vocab, size=2900).tolist()
    gens = {}
    for arm in ("bf16", "fp8", "mxfp4"):
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
        raise SystemExit("w4_decode.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    res = {"bench": "w4_decode", "gemv": gemv_arms(dev, a.rounds)}
    if not a.skip_model:
        res["phi3_mini_b1"] = model_arms(dev, a.model_rounds)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
