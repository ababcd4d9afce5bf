// What the decode-attention kernels share (decode_attn.hip: bf16 cache; decode_kv8.hip: fp8 cache).
// Device side, the split-KV merge machinery: keys per split, the per-split store, the in-kernel merge
// by the last split of a (row, kv head) pair, and the separate combine kernel. Host side (at the end):
// the launch arguments (DecArgs), their checks (dec_fill) and the combine launch (dec_combine).
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

// ---- host: one launch's arguments, cache operands excepted (each file derives its own struct) ----
struct DecArgs {
  const bf16_t* q; const int* lens; const int* slot; const int* pre;
  int ldq, B, H, Hkv, G, D, max_seq, chunk, nsplit, ldo;
  float sl2e;                        // scale * log2(e)
  float* po; float* pm; float* pl;   // split partials in ws: po [B, H, nsplit, D], pm / pl [B, H, nsplit]
  bf16_t* out; int* cnt;
  dim3 grid;                         // (nsplit, Hkv, B)
  hipStream_t s;
};
// the decode kernels' parameters that follow (q, ldq, <cache operands>)
#define DEC_KARGS(a) (a).lens, (a).slot, (a).pre, (a).H, (a).Hkv, (a).max_seq, (a).chunk, (a).nsplit, (a).sl2e, (a).po, \
                     (a).pm, (a).pl, (a).out, (a).ldo, (a).cnt

// Checks what every decode kernel relies on and fills the arguments; the cache pointers are the
// caller's to check. 0, or hipErrorInvalidValue: refused. B == 0 passes (nothing to launch).
// ws must hold B*H*nsplit*(D+2) floats. chunk = keys per split (multiple of 64).
// pre (nullable): int32 [B][2] = (P, prefix slot) per row — keys [0, P) of row b are read from the
// prefix slot (a prompt head shared by the whole batch, stored once; the decoder passes whole 64-key
// tiles, and the one tile that straddles the two sources at any other P selects its source per key). Every row of the batch reads the same prefix lines, so they are served
// from L2 / MALL instead of HBM.
// counters (nullable): int32 [B * Hkv], all zero, left zero by every launch -> the splits are merged
// inside the attention kernel (last split per (b, kv head)); null -> separate combine launch. With
// counters, ws and counters must be uncached allocations (da_malloc_uncached).
// cos_sin / pos (both null, or both set): fused RoPE + new-token KV-cache write (bf16 cache, MHA
// only; q is then the raw qkv row, see DecRope).
static inline int dec_fill(DecArgs& a, const void* q, int ldq, const void* lens, const void* slot, const void* pre,
                           int B, int H, int Hkv, int D, int max_seq, int chunk, int nsplit, float scale, void* ws,
                           void* o, int ldo, void* counters, const void* cos_sin, const void* pos, void* stream) {
  bool ok = Hkv >= 1 && H % Hkv == 0 && chunk >= 64 && chunk % 64 == 0 && nsplit >= 1 && (D == 64 || D == 96 || D == 128);
  ok = ok && q && lens && slot && o && (nsplit == 1 || ws);
  ok = ok && (cos_sin == nullptr) == (pos == nullptr) && (!cos_sin || (H == Hkv && ldq >= (H + 2 * Hkv) * D));
  if (!ok) return (int)hipErrorInvalidValue;
  a.q = (const bf16_t*)q; a.lens = (const int*)lens; a.slot = (const int*)slot; a.pre = (const int*)pre;
  a.ldq = ldq; a.B = B; a.H = H; a.Hkv = Hkv; a.G = H / Hkv; a.D = D; a.max_seq = max_seq; a.chunk = chunk;
  a.nsplit = nsplit; a.ldo = ldo;
  a.sl2e = scale * 1.4426950408889634f;
  a.po = (float*)ws; a.pm = a.po + (size_t)B * H * nsplit * D; a.pl = a.pm + (size_t)B * H * nsplit;
  a.out = (bf16_t*)o; a.cnt = (int*)counters;
  a.grid = dim3(nsplit, Hkv, B); a.s = (hipStream_t)stream;
  return 0;
}

// The separate merge of the splits, when the kernel did not do it (no counters).
static inline int dec_combine(const DecArgs& a) {
  if (a.nsplit == 1 || a.cnt) return 0;
#define DEC_COMBINE(DD, NT) decode_combine_kernel<DD><<<dim3(a.H, a.B), NT, 0, a.s>>>(a.po, a.pm, a.pl, a.H, a.nsplit, a.out, a.ldo)
  if (a.D == 64) DEC_COMBINE(64, 64); else if (a.D == 96) DEC_COMBINE(96, 128); else DEC_COMBINE(128, 128);
#undef DEC_COMBINE
  DA_LAUNCH_CHECK();
}
