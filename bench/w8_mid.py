"""fp8 (e4m3) decoder weights vs bf16 at 33..128 rows, one process, arms interleaved (the method of
bench/w8_dk.py: a 1 GiB pool of weight copies per arm so every launch streams cold weights, one
captured graph per pass, median of the rounds; the bf16 arm runs twice per round, "bf16" and "bf16_b":
their ratio is the run-to-run spread a loss has to exceed):
(a) the five Phi-3-mini products at M = 40, 64, 96, 128 as the decode step runs them. 40 / 64 rows
    (the gemm_dk-structured step): kernels.gemm_dk on the dequantised bf16 weights (its split-K
    route) vs kernels.gemm_dk_splitk_w8, QKV / gate-up / LM head with the deferred norm, O / down with
    residual + row sums. 96 / 128 rows (the fused-norm step): kernels.gemm vs kernels.gemm_tile_w8
    (QKV, gate-up, LM head), kernels.gemm_resid_norm vs kernels.gemm_resid_norm_w8 (O, down). us per
    launch. --nt adds the fp8 arm with the non-temporal code loads forced off / on ("fp8_nt0",
    "fp8_nt1"; "fp8" is the library's per-tile rule).
(b) --kv bf16|fp8: the graph-replayed Phi-3-mini decode step (real dims, random weights, 512 cached
    tokens per row) at batch 64 and 128 with that KV cache: LlamaDecoder(weight_dtype="fp8") vs a bf16
    decoder on a deep copy of the dequantised weights; ms per step.
One JSON line per table row."""
import argparse
import copy
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from docagents_amd.ops import kernels as K  # noqa: E402
from w8_decode import POOL_BYTES, graph_of, pool, time_graphs  # noqa: E402
from w8_dk import step_graph  # noqa: E402

EPS = 1e-5
ROWS = (40, 64, 96, 128)
STEP_ROWS = (64, 128)
SHAPES = [("qkv", 9216, 3072, K.EPI_NONE), ("o", 3072, 3072, K.EPI_RESID), ("gate_up", 16384, 3072, K.EPI_SWIGLU),
          ("down", 3072, 8192, K.EPI_RESID), ("lm_head", 32064, 3072, K.EPI_NONE)]


def launchers(M, N, Kd, epi, dev):
    """(dq, q, s, bf16 launch(w), fp8 launch(wq)) of one product as the M-row decode step runs it."""
    g = torch.Generator(device=dev).manual_seed(N + Kd + M)
    w = (torch.randn(N, Kd, device=dev, generator=g) * Kd ** -0.5).to(torch.bfloat16)
    q, s = K.quant_weight_fp8_pow2(w)
    dq = (q.float() * s[:, None]).to(torch.bfloat16)
    x = torch.randn(M, Kd, device=dev, generator=g).to(torch.bfloat16)
    resid = torch.randn(M, N, device=dev, generator=g).to(torch.bfloat16) if epi == K.EPI_RESID else None
    out = torch.empty((M, N // 2 if epi == K.EPI_SWIGLU else N), dtype=torch.bfloat16, device=dev)
    if M <= K.DK_MAX_M:
        kw = dict(epi=epi, resid=resid, out=out)
        if epi == K.EPI_RESID:
            kw["ssq_out"] = torch.zeros(512 * 64, dtype=torch.float32, device=dev)
        else:  # one part holding the rows' sums of squares: the reduce only sums the parts it is told
            ssq = torch.zeros(512 * 64, dtype=torch.float32, device=dev)
            ssq.view(-1, 64)[0, :M] = x.float().pow(2).sum(-1)
            kw["norm_in"] = (ssq, K.dk_parts(Kd, M), EPS)
        return dq, q, s, out, (lambda wb: K.gemm_dk(x, wb, **kw)), (lambda w8: K.gemm_dk_splitk_w8(x, w8, s, **kw))
    if epi == K.EPI_RESID:
        gamma, h = torch.ones(N, dtype=torch.bfloat16, device=dev), torch.empty_like(resid)
        return (dq, q, s, out, (lambda wb: K.gemm_resid_norm(x, wb, resid, gamma, EPS, out=out, h_out=h)),
                (lambda w8: K.gemm_resid_norm_w8(x, w8, s, resid, gamma, EPS, out=out, h_out=h)))
    return dq, q, s, out, (lambda wb: K.gemm(x, wb, epi=epi, out=out)), (lambda w8: K.gemm_tile_w8(x, w8, s, epi=epi, out=out))


def product_arms(dev, rounds, nt):
    for name, N, Kd, epi in SHAPES:
        for M in ROWS:
            dq, q, s, out, run_b, run_8 = launchers(M, N, Kd, epi, dev)
            nb, n8 = max(2, POOL_BYTES // (N * Kd * 2)), max(2, POOL_BYTES // (N * Kd))
            wb, w8 = pool(dq, nb), pool(q, n8)
            run_b(wb[0])
            want = out.clone()
            graphs = {"bf16": graph_of(lambda i: run_b(wb[i]), nb), "fp8": graph_of(lambda i: run_8(w8[i]), n8),
                      "bf16_b": graph_of(lambda i: run_b(wb[i]), nb)}
            n = {"bf16": nb, "fp8": n8, "bf16_b": nb}
            if nt:
                for v in (0, 1):  # the load policy is picked at launch: captured with the graph
                    K.gemm_tile_w8_nt(v)
                    graphs[f"fp8_nt{v}"] = graph_of(lambda i: run_8(w8[i]), n8)
                    n[f"fp8_nt{v}"] = n8
                K.gemm_tile_w8_nt(-1)
            run_8(w8[0])
            torch.cuda.synchronize()
            assert torch.equal(out, want), (name, M)  # the fp8 arm: the bf16 arm's bits
            t = time_graphs(graphs, n, rounds)
            row = {"shape": name, "M": M, "N": N, "K": Kd, "us": {k: round(v[0], 2) for k, v in t.items()},
                   "us_min": {k: round(v[1], 2) for k, v in t.items()},
                   "fp8_over_bf16": round(t["fp8"][0] / t["bf16"][0], 3),
                   "bf16_b_over_bf16": round(t["bf16_b"][0] / t["bf16"][0], 3)}
            print(json.dumps(row), flush=True)
            del graphs, wb, w8
            torch.cuda.empty_cache()


def model_arms(dev, rounds, kv, steps=16, ctx=512):
    from docagents_amd.models.configs import decoder_config
    from docagents_amd.models.llama import LlamaDecoder
    cfg = decoder_config("phi3-mini")
    f = LlamaDecoder(cfg, dev, seed=0, weight_dtype="fp8", kv_dtype=kv)
    strip = lambda d: {k: v for k, v in d.items() if not k.endswith(("_q8", "_s8")) and k != "layers"}  # noqa: E731
    wb = copy.deepcopy({**strip(f.w), "layers": [strip(L) for L in f.w["layers"]]})
    b = LlamaDecoder(cfg, dev, weights=wb, kv_dtype=kv)
    for m in (f, b):
        m.alloc_cache(max(STEP_ROWS), ctx + 128)
    for B in STEP_ROWS:
        arms = {"bf16": step_graph(b, B, ctx), "fp8": step_graph(f, B, ctx), "bf16_b": step_graph(b, B, ctx)}
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
        row = {"phi3_mini_step": True, "B": B, "ctx": ctx, "kv": kv,
               "ms_per_step": {k: round(float(np.median(v)), 4) for k, v in ms.items()},
               "ms_per_step_min": {k: round(float(np.min(v)), 4) for k, v in ms.items()}}
        row["fp8_over_bf16"] = round(row["ms_per_step"]["fp8"] / row["ms_per_step"]["bf16"], 3)
        row["bf16_b_over_bf16"] = round(row["ms_per_step"]["bf16_b"] / row["ms_per_step"]["bf16"], 3)
        print(json.dumps(row), flush=True)
        del arms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--nt", action="store_true", help="add the fp8 arm with non-temporal code loads forced off / on")
    ap.add_argument("--kv", choices=("bf16", "fp8"), help="measure the decode step with this KV cache instead of the products")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("w8_mid.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    K.reserve_workspace(256 << 20, dev)  # a workspace that grew would free the buffer captured graphs point at
    if a.kv:
        model_arms(dev, a.rounds, a.kv)
    else:
        product_arms(dev, a.rounds, a.nt)


if __name__ == "__main__":
    main()
