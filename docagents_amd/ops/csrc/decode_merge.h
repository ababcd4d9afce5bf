// Split-KV merge machinery shared by the decode-attention kernels (attention.hip: bf16 cache;
// decode_kv8.hip: fp8 cache): keys per split, the per-split store, the in-kernel merge by the last
// split of a (row, kv head) pair, and the separate combine kernel.
#pragma once
#include "common.h"

// Split-KV epilogue shared by the decode kernels. A split's merged (over its 4 waves) result for
// query head h: unnormalised O row `o`, running max M (log2 domain), sum ls. With one split the
// normalised bf16 output is written directly; otherwise the fp32 partial, and the LAST split of
// (b, kv head) to finish (atomic ticket in cnt[b * Hkv + hk], reset by that split so the counters
// are zero again for the next launch / graph replay) merges all splits of its G heads — the
// separate combine launch (~5 us per layer, most of a batch-1 decode attention) is gone.
// Keys per split of a row. The grid's split count is fixed at capture (sized for the cache
// capacity, max_len), but a row holds L <= max_len keys: balanced splits (the default) spread the
// row's L keys over ALL its splits (64-key multiples) instead of filling the first ceil(L / chunk)
// and leaving the rest idle — at batch 1 and 2.9k of 4k keys, 256 working workgroups instead of 192.
__device__ __forceinline__ int dec_chunk(int L, int nsplit, int chunk_arg) {
  const int c = ((L + nsplit - 1) / nsplit + 63) & ~63;
  return c < chunk_arg ? c : chunk_arg;
}

__device__ __forceinline__ void dec_store(float o, float M, float ls, int b, int h, int d, int H, int nsplit,
                                          int split, int D, float* po, float* pm, float* pl, bf16_t* out,
                                          int ldo) {
  if (nsplit == 1) {
    out[(size_t)b * ldo + h * D + d] = f2bf(ls > 0.f ? o / ls : 0.f);
    return;
  }
  const size_t pidx = ((size_t)b * H + h) * nsplit + split;
  po[pidx * D + d] = o;
  if (d == 0) { pm[pidx] = M; pl[pidx] = ls; }
}

// XC (same-XCD exchange): every split of (b, kv head) ran on ONE XCD (the launch's workgroup ->
// XCD round-robin, see decode_attn_kernel), so partials and tickets live in ordinary (cached)
// memory: the stores reach that XCD's L2, the ticket is an L2 atomic and the merging split reads
// the partials from L2 (agent-scope loads: past its L1) — L2 round trips instead of uncached ones.
template <int D, int G, bool XC = false>
__device__ __forceinline__ void dec_finish(const float* po, const float* pm, const float* pl, int H, int Hkv,
                                           int nsplit, int b, int hk, int* cnt, bf16_t* out, int ldo, int* s_last) {
  if (nsplit == 1 || cnt == nullptr) return;  // no counters: the host launches decode_combine_kernel
  const int tid = threadIdx.x;
  // Partials and tickets live in UNCACHED memory (da_malloc_uncached: MTYPE UC, L2 bypassed), so
  // device-wide visibility needs only this workgroup's stores to have completed — no
  // __threadfence(), whose L2 write-back + invalidate of the whole cache costs more than the
  // combine launch it replaces (measured: 24.6 -> 48.4 us at batch 1).
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    int* c = &cnt[b * Hkv + hk];
    const int old = XC ? __hip_atomic_fetch_add(c, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : atomicAdd(c, 1);
    *s_last = old == nsplit - 1;
    if (*s_last) {
      if constexpr (XC) __hip_atomic_store(c, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else *c = 0;
    }
  }
  __syncthreads();
  if (!*s_last) return;
  auto ld = [](const float* p) -> float {
    if constexpr (XC) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return *p;
  };
  // One online pass over the splits, 8 splits' (m, l, o) loads issued per step: the partials sit in
  // uncached memory (~1-2 us per round trip), so a max pass + a sum pass that each walk the splits
  // one dependent load at a time cost ~2 x nsplit round trips — most of a batch-1 decode attention.
  for (int i = tid; i < G * D; i += blockDim.x) {
    const int g = i / D, d = i % D, h = hk * G + g;
    const size_t base = ((size_t)b * H + h) * nsplit;
    float M = -INFINITY, lsum = 0.f, acc = 0.f;
    for (int s0 = 0; s0 < nsplit; s0 += 8) {
      float ms[8], ls[8], os[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int s = min(s0 + j, nsplit - 1);
        ms[j] = ld(pm + base + s);
        ls[j] = ld(pl + base + s);
        os[j] = ld(po + (base + s) * D + d);
      }
      float mx = M;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (s0 + j < nsplit) mx = fmaxf(mx, ms[j]);
      const float mu = (mx == -INFINITY) ? 0.f : mx;
      const float r = (M == -INFINITY) ? 0.f : exp2f(M - mu);
      lsum *= r;
      acc *= r;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (s0 + j >= nsplit) continue;
        const float f = exp2f(ms[j] - mu);
        lsum += ls[j] * f;
        acc += os[j] * f;
      }
      M = mx;
    }
    out[(size_t)b * ldo + h * D + d] = f2bf(lsum > 0.f ? acc / lsum : 0.f);
  }
}

template <int D>
__global__ void decode_combine_kernel(const float* __restrict__ po, const float* __restrict__ pm,
                                      const float* __restrict__ pl, int H, int nsplit, bf16_t* __restrict__ o,
                                      int ldo) {
  const int b = blockIdx.y, h = blockIdx.x;
  const size_t base = ((size_t)b * H + h) * nsplit;
  float M = -INFINITY;
  for (int s = 0; s < nsplit; ++s) M = fmaxf(M, pm[base + s]);
  const float Mu = (M == -INFINITY) ? 0.f : M;
  float lsum = 0.f;
  for (int s = 0; s < nsplit; ++s) lsum += pl[base + s] * exp2f(pm[base + s] - Mu);
  const float inv = lsum > 0.f ? 1.f / lsum : 0.f;
  for (int d = threadIdx.x; d < D; d += blockDim.x) {
    float acc = 0.f;
    for (int s = 0; s < nsplit; ++s) acc += po[(base + s) * D + d] * exp2f(pm[base + s] - Mu);
    o[(size_t)b * ldo + h * D + d] = f2bf(acc * inv);
  }
}
