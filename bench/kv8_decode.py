"""fp8 (e4m3) KV cache vs bf16, one process, arms interleaved round by round:
(a) the decode-attention launch at Phi-3 width (H = Hkv = 32, D = 96, ~2.9k of 4096 keys per row) at
    batch 128 and batch 1: kernels.decode_attn on a bf16 cache vs kernels.decode_attn_kv8 on its
    quantisation (+ the rope_cache_kv8 launch the fp8 decode step adds, timed on its own). Launches
    replay from one captured graph; at batch 1 every launch of a pass reads another slot, so the
    256 MB Infinity Cache never holds the keys. us per launch and TB/s from the bytes the shapes imply.
(b) Phi-3-mini (real dims, random weights), LlamaDecoder(kv_dtype="bf16") vs ("fp8") on shared
    weights: Generator.generate of 128 QA-sized prompts (a shared 260-token head + ~2.6k tokens) and
    of one: graph-replayed decode ms per step and the prefill wall time of the 128-prompt chunk.
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

H = HKV = 32
D = 96
MAX_LEN = 4096
LEN = 2932  # 2900 + the middle of a 64-token answer


def graph_of(launch, n):
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


def time_graphs(graphs, n, rounds):
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
        us = np.array([a.elapsed_time(b) * 1e3 / n for a, b in pairs])
        out[k] = (float(np.median(us)), float(us.min()))
    return out


def launch_arms(dev, B, rounds):
    """B rows per launch; the cache holds `passes` groups of B slots and launch i reads group i."""
    passes = 2 if B > 1 else 16  # 2 x 6.4 GB of bf16 keys at batch 128; 16 x 50 MB at batch 1
    slots = B * passes
    g = torch.Generator(device=dev).manual_seed(B)
    kv = torch.empty(2, slots, HKV, MAX_LEN, D, dtype=torch.bfloat16, device=dev)
    for i in range(2):
        for s in range(slots):  # slot by slot: no fp32 copy of the whole cache
            kv[i, s] = torch.randn(HKV, MAX_LEN, D, device=dev, generator=g).to(torch.bfloat16)
    codes = torch.empty(2, slots, HKV, MAX_LEN, D, dtype=torch.uint8, device=dev).view(K.FP8)
    scales = torch.empty(2, slots, HKV, MAX_LEN, dtype=torch.float32, device=dev)
    for i in range(2):
        for s in range(slots):
            q8, s8 = K.quant_weight_fp8_pow2(kv[i, s].reshape(-1, D))
            codes[i, s] = q8.view(HKV, MAX_LEN, D)
            scales[i, s] = s8.view(HKV, MAX_LEN)
    qkv = torch.randn(B, (H + 2 * HKV) * D, device=dev, generator=g).to(torch.bfloat16)
    lens = torch.full((B,), LEN, dtype=torch.int32, device=dev)
    pos = lens - 1
    slot = [(torch.arange(B, device=dev) + i * B).int() for i in range(passes)]
    out = torch.empty(B, H * D, dtype=torch.bfloat16, device=dev)
    cs = torch.zeros(MAX_LEN, D // 2, 2, dtype=torch.float32, device=dev)
    cs[..., 0] = 1.0  # identity rotation: the timing does not depend on the angles
    graphs = {
        "bf16": graph_of(lambda i: K.decode_attn(qkv, kv[0], kv[1], lens, slot[i], H, HKV, D, MAX_LEN, out=out), passes),
        "bf16_fused_rope": graph_of(lambda i: K.decode_attn(qkv, kv[0], kv[1], lens, slot[i], H, HKV, D, MAX_LEN, out=out,
                                                            rope=(cs, pos)), passes),
        "fp8": graph_of(lambda i: K.decode_attn_kv8(qkv, codes[0], codes[1], scales[0], scales[1], lens, slot[i], H, HKV,
                                                    D, MAX_LEN, out=out), passes),
        "fp8_rope_write": graph_of(lambda i: K.rope_cache_kv8(qkv, pos, cs, H, HKV, D, slot[i], codes[0], codes[1],
                                                              scales[0], scales[1]), passes),
    }
    t = time_graphs(graphs, passes, rounds)
    nbytes = {"bf16": B * HKV * LEN * D * 2 * 2, "bf16_fused_rope": B * HKV * LEN * D * 2 * 2,
              "fp8": B * HKV * LEN * (D + 4) * 2}
    r = {"B": B, "lens": LEN, "max_len": MAX_LEN}
    for arm, (med, mn) in t.items():
        r[arm] = {"us": round(med, 2), "us_min": round(mn, 2)}
        if arm in nbytes:
            r[arm]["TBps"] = round(nbytes[arm] / med / 1e6, 2)
    r["fp8_over_bf16"] = round(t["fp8"][0] / t["bf16"][0], 3)
    r["fp8_plus_write_over_bf16_fused"] = round((t["fp8"][0] + t["fp8_rope_write"][0]) / t["bf16_fused_rope"][0], 3)
    del graphs, kv, codes, scales
    torch.cuda.empty_cache()
    return r


def model_arms(dev, rounds, batch, new, max_seq):
    from docagents_amd.engine.generator import Generator
    from docagents_amd.models.configs import decoder_config
    from docagents_amd.models.llama import LlamaDecoder
    cfg = decoder_config("phi3-mini")
    rng = np.random.default_rng(0)
    head = rng.integers(300, cfg.vocab, size=260).tolist()
    many = [head + rng.integers(300, cfg.vocab, size=2640 - 16 * (i % 8)).tolist() for i in range(batch)]
    gens, w = {}, None
    for arm in ("bf16", "fp8"):
        m = LlamaDecoder(cfg, dev, seed=0, weights=w, kv_dtype=arm)
        w = m.w
        m.alloc_cache(batch + 2, max_seq)
        gens[arm] = Generator(m, max_batch=batch, max_seq=max_seq, temperature=0.2, seed=3, eos=())
        gens[arm].sync_phases = True
    res = {arm: {} for arm in gens}
    for name, prompts in ((f"b{batch}", many), ("b1", many[:1])):
        step_ms = {k: [] for k in gens}
        pf_ms = {k: [] for k in gens}
        for rnd in range(rounds + 1):
            for arm, g in gens.items():
                d0, n0 = g.stats["decode_s"], g.stats["decode_steps"]
                p0 = g.stats.get("prefill_wall_s", 0.0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = g.generate(prompts, new)
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
                assert all(len(o.tokens) == new for o in out)
                if rnd > 0:  # round 0 captures the graphs
                    step_ms[arm].append((g.stats["decode_s"] - d0) * 1e3 / max(1, g.stats["decode_steps"] - n0))
                    pf_ms[arm].append((g.stats.get("prefill_wall_s", 0.0) - p0) * 1e3)
                    res[arm][f"{name}_generate_ms"] = round(wall * 1e3, 1)
        for arm in gens:
            res[arm][f"{name}_decode_ms_per_step"] = round(float(np.median(step_ms[arm])), 4)
            res[arm][f"{name}_prefill_ms"] = round(float(np.median(pf_ms[arm])), 2)
    res["config"] = {"batch": batch, "new": new, "max_seq": max_seq, "prompt_tokens": len(many[0])}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--model-rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--new", type=int, default=32)
    ap.add_argument("--max-seq", type=int, default=3072)  # both arms' caches side by side: 157 + 82 GB
    ap.add_argument("--skip-model", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kv8_decode.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    res = {"bench": "kv8_decode", "launch_b128": launch_arms(dev, 128, a.rounds), "launch_b1": launch_arms(dev, 1, a.rounds)}
    print(json.dumps(res), flush=True)
    if not a.skip_model:
        res["phi3_mini"] = model_arms(dev, a.model_rounds, a.batch, a.new, a.max_seq)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
