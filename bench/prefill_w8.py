"""fp8 (W8A8) prefill against the bf16 prefill (LLM_PREFILL_DTYPE), one process, arms interleaved:
every round times the bf16 arm and then the fp8 arm (device events around `iters` launches); the
figures are the median over the rounds, with each arm's min and max as the run-to-run spread.
(a) --products: the four products of a prefill layer, Phi-3-mini shapes at M = 2930 (batch-1 prefill),
    29440 and 32768, Llama-3-8B's at M = 8192. bf16 arm: what LlamaDecoder.prefill runs today, the
    RMSNorm it needs included (rmsnorm + gemm_rope; gemm EPI_RESID; rmsnorm + gemm EPI_SWIGLU; gemm
    EPI_RESID). fp8 arm: the quantisation always included (rmsnorm_q8 + gemm_fp8 + rope_cache;
    quant_fp8 + gemm_fp8 EPI_RESID; rmsnorm_q8 + gemm_fp8 EPI_SWIGLU; quant_fp8 + gemm_fp8 EPI_RESID).
    TF/s counts 2 M N K over the arm's whole time (an end-to-end figure of the arm, not a kernel's).
(b) --model: Phi-3-mini (real dims, random weights, weight_dtype="fp8" in both arms), the whole
    prefill of 128 QA-sized prompts (29440 rows) and of one 2930-token prompt, prefill_dtype fp8
    against bf16, with the bf16 and the fp8 KV cache; then the accuracy of the fp8 prefill against
    the bf16 prefill of the same model: max and mean |dlogit|, share of equal greedy first tokens.
One JSON line per row."""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from docagents_amd.ops import kernels as K  # noqa: E402

EPS = 1e-5
# name, N, K, epilogue; heads / kv heads / head dim for the QKV product's RoPE + cache write
PHI3 = dict(name="phi3-mini", H=32, Hkv=32, D=96, rows=(2930, 29440, 32768),
            shapes=[("qkv", 9216, 3072, K.EPI_NONE), ("o", 3072, 3072, K.EPI_RESID),
                    ("gate_up", 16384, 3072, K.EPI_SWIGLU), ("down", 3072, 8192, K.EPI_RESID)])
LLAMA8B = dict(name="llama3-8b", H=32, Hkv=8, D=128, rows=(8192,),
               shapes=[("qkv", 6144, 4096, K.EPI_NONE), ("o", 4096, 4096, K.EPI_RESID),
                       ("gate_up", 28672, 4096, K.EPI_SWIGLU), ("down", 4096, 14336, K.EPI_RESID)])


def time_arms(arms, rounds, iters):
    """{name: fn} -> {name: (median, min, max) ms per call}; one untimed round first."""
    ms = {k: [] for k in arms}
    for rnd in range(rounds + 1):
        for k, fn in arms.items():
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            e.record()
            torch.cuda.synchronize()
            if rnd > 0:
                ms[k].append(a.elapsed_time(e) / iters)
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in ms.items()}


def product_arms(model, dev, rounds):
    H, Hkv, D = model["H"], model["Hkv"], model["D"]
    g = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, device=dev, generator=g) * scale).to(torch.bfloat16)  # noqa: E731
    cs = None
    for M in model["rows"]:
        for name, N, Kd, epi in model["shapes"]:
            wq, sw = K.quant_weight_fp8_pow2(rnd(N, Kd, scale=Kd ** -0.5))
            w = (wq.float() * sw[:, None]).to(torch.bfloat16)  # the model both arms compute
            x, gain = rnd(M, Kd), torch.ones(Kd, dtype=torch.bfloat16, device=dev)
            nout = N // 2 if epi == K.EPI_SWIGLU else N
            out = torch.empty(M, nout, dtype=torch.bfloat16, device=dev)
            resid = rnd(M, N) if epi == K.EPI_RESID else None
            codes = torch.empty(M, Kd, dtype=K.FP8, device=dev)
            scale = torch.empty(M, dtype=torch.float32, device=dev)
            h = torch.empty(M, Kd, dtype=torch.bfloat16, device=dev)
            if name == "qkv":
                from docagents_amd.ops.reference import rope_table
                S = 512
                slots = -(-M // S)
                kc = torch.zeros(slots, Hkv, S, D, dtype=torch.bfloat16, device=dev)
                vc = torch.zeros_like(kc)
                pos = (torch.arange(M, device=dev) % S).to(torch.int32)
                slot = (torch.arange(M, device=dev) // S).to(torch.int32)
                cs = rope_table(S, D, 10000.0, dev)
                kv_out = not K.flash_kv_cache_ok(D, True)  # as LlamaDecoder.prefill asks

                def bf16():
                    K.rmsnorm(x, gain, EPS, out=h)
                    K.gemm_rope(h, w, pos, cs, H, Hkv, D, slot, kc, vc, out=out, kv_out=kv_out)

                def fp8():
                    K.rmsnorm_q8(x, gain, EPS, out=codes, scale=scale)
                    K.gemm_fp8(codes, scale, wq, sw, out=out)
                    K.rope_cache(out, pos, cs, H, Hkv, D, slot=slot, k_cache=kc, v_cache=vc)
            elif epi == K.EPI_SWIGLU:
                def bf16():
                    K.rmsnorm(x, gain, EPS, out=h)
                    K.gemm(h, w, epi=epi, out=out)

                def fp8():
                    K.rmsnorm_q8(x, gain, EPS, out=codes, scale=scale)
                    K.gemm_fp8(codes, scale, wq, sw, epi=epi, out=out)
            else:
                def bf16():
                    K.gemm(x, w, epi=epi, resid=resid, out=out)

                def fp8():
                    K.quant_fp8(x, out=codes, scale=scale)
                    K.gemm_fp8(codes, scale, wq, sw, epi=epi, resid=resid, out=out)
            flop = 2.0 * M * N * Kd
            iters = max(4, min(400, int(6e13 / flop)))  # >= ~40 ms of work per timed window
            t = time_arms({"bf16": bf16, "fp8": fp8}, rounds, iters)
            row = {"model": model["name"], "product": name, "M": M, "N": N, "K": Kd, "iters": iters, "rounds": rounds}
            for k, (med, lo, hi) in t.items():
                row[k] = {"us": round(med * 1e3, 1), "us_min": round(lo * 1e3, 1), "us_max": round(hi * 1e3, 1),
                          "tflops": round(flop / (med * 1e-3) / 1e12, 1)}
            row["fp8_over_bf16"] = round(t["fp8"][0] / t["bf16"][0], 3)
            # the arms' ranges do not overlap: the difference is larger than the run-to-run spread
            row["separated"] = bool(t["fp8"][2] < t["bf16"][1] or t["bf16"][2] < t["fp8"][1])
            print(json.dumps(row), flush=True)
            del wq, sw, w, x, out, resid, codes, scale, h
            torch.cuda.empty_cache()


def _packed(prompts, dev):
    from docagents_amd.models.llama import pack_prompts
    flat, pos, cu, lens = pack_prompts(prompts)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    slot_tok = np.repeat(np.arange(len(prompts), dtype=np.int32), lens)
    return (to(flat), to(pos), to(slot_tok), to(cu), int(lens.max()), to((cu[1:] - 1).astype(np.int64)))


def model_arms(dev, rounds):
    from docagents_amd.models.configs import decoder_config
    from docagents_amd.models.llama import LlamaDecoder
    cfg = decoder_config("phi3-mini")
    f = LlamaDecoder(cfg, dev, seed=0, weight_dtype="fp8", prefill_dtype="fp8")
    b = LlamaDecoder(cfg, dev, weights=f.w, weight_dtype="fp8")  # the same tensors: one model, two prefills
    rng = np.random.default_rng(0)
    lens = rng.integers(200, 261, size=128)
    lens[-1] += 29440 - int(lens.sum())  # 128 QA-sized prompts, 29440 rows in all
    qa = [[int(t) for t in rng.integers(5, cfg.vocab - 5, size=n)] for n in lens]
    one = [[int(t) for t in rng.integers(5, cfg.vocab - 5, size=2930)]]
    logits = {}
    for what, prompts, max_seq in (("qa128", qa, 512), ("one2930", one, 3072)):
        args = _packed(prompts, dev)
        for kv in ("bf16", "fp8"):
            for m in (b, f):  # the bench's own switch of the cache type: both decoders share one cache
                m.kv_dtype = kv
            f.alloc_cache(len(prompts), max_seq)
            b.cache = f.cache
            arms = {"bf16": lambda: b.prefill(*args), "fp8": lambda: f.prefill(*args)}
            t = time_arms(arms, rounds, 1)
            row = {"prefill": what, "rows": int(args[0].numel()), "kv": kv, "rounds": rounds}
            for k, (med, lo, hi) in t.items():
                row[k] = {"ms": round(med, 2), "ms_min": round(lo, 2), "ms_max": round(hi, 2)}
            row["fp8_over_bf16"] = round(t["fp8"][0] / t["bf16"][0], 3)
            row["separated"] = bool(t["fp8"][2] < t["bf16"][1] or t["bf16"][2] < t["fp8"][1])
            print(json.dumps(row), flush=True)
            if kv == "bf16":
                logits[what] = (b.prefill(*args).float(), f.prefill(*args).float())
            f.cache = b.cache = None
            torch.cuda.empty_cache()
    for what, (lb, lf) in logits.items():
        d = (lf - lb).abs()
        print(json.dumps({"accuracy": what, "prompts": int(lb.shape[0]), "max_abs_dlogit": round(float(d.max()), 4),
                          "mean_abs_dlogit": round(float(d.mean()), 5),
                          "logit_abs_mean": round(float(lb.abs().mean()), 4),
                          "rel_l2": round(float((lf - lb).norm() / lb.norm()), 4),
                          "greedy_first_token_agree": round(float((lf.argmax(-1) == lb.argmax(-1)).float().mean()), 4)}),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--products", action="store_true")
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prefill_w8.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    if a.products or not a.model:
        for model in (PHI3, LLAMA8B):
            product_arms(model, dev, a.rounds)
    if a.model or not a.products:
        model_arms(dev, max(3, a.rounds // 2))


if __name__ == "__main__":
    main()
