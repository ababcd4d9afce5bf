// Decode attention for gfx950 (one new token per sequence) over the bf16 KV cache
// [slot, Hkv, max_seq, D]: split-KV ("flash-decoding") so a batch of long contexts fills all 256
// CUs; fp32 partials (unnormalised O, running max, running sum) merged by the last split of a
// (row, kv head) pair or by decode_combine (decode_merge.h). Three kernels, one host route (dec_route).
#include "common.h"
#include "decode_merge.h"  // dec_chunk / dec_store / dec_finish / DecArgs / dec_fill / dec_combine

#include <cstdlib>
#include <type_traits>

// Floating-point contraction only within one expression (a*b + c -> fma), never across statements:
// with the HIP default (fast) the backend fuses differently depending on the code around an expression
// (a copy of this attention inlined into another kernel once differed by one bf16 ulp on some heads).
// Pinned, an expression's bits do not depend on the surrounding code: every instance rounds alike.
#pragma clang fp contract(on)

// decode_attn_kernel's VAR template argument is a set of these bits (explained in the kernel).
constexpr int DEC_NT = 1;      // non-temporal K / V loads
constexpr int DEC_VEARLY = 2;  // V issued together with K
constexpr int DEC_PFT = 4;     // the wave's next tile prefetched (implies VEARLY)
constexpr int DEC_XC = 8;      // same-XCD split exchange

// ------------------------------------------------------------------------------------------
// Decode attention: q [B, ldq] (head h at h*D), caches [slots, Hkv, max_seq, D],
// lens[b] = tokens in cache for b (current token included), slot[b] = cache slot of b.
// Partials: po [B, H, nsplit, D] fp32 (unnormalised, relative to pm), pm/pl [B, H, nsplit].
//
// Memory-bound streaming design: for a fixed (slot, kv head) the keys of a 64-key tile are one
// contiguous [64 x D] bf16 block, so each wave loads it as a flat byte array with fully coalesced
// 16-B-per-lane loads (1 KiB per wave-instruction) — chunk c = 64*i + lane holds key c / (D/8),
// dims 8*(c % (D/8)) .. +7. Partial dot products are reduced per key with lane shuffles when a key's
// chunks sit in one wave-instruction (D = 64, 128) or through a small per-wave LDS buffer (D = 96).
// The P*V accumulation uses the same flat chunks: lane's dim-slot for chunk i is static given
// i mod NSET, so accumulators stay in registers. Each of the 4 waves streams its own tiles with its
// own online softmax (no block barriers in the loop); the waves are merged once at the end.
// Fused RoPE + KV-cache write for the decode step (cs != null; MHA kernel): q is the raw qkv row
// ([q heads | k heads | v heads], row stride ldq). The kernel rotates q on its way into LDS, and
// the split holding the new token (key L-1, rope position pos[b] == L-1) takes that key's rotated
// k and v straight from the qkv row — as one extra online-softmax term, never read back from the
// cache — and writes them into the cache slot for later steps. Replaces the per-layer
// rope_cache launch of the decode step (bit-identical: the same bf16 roundings).
struct DecRope {
  bf16_t* kc;           // cache bases (writable) for the new token's k / v
  bf16_t* vc;
  const float* cs;      // [max_pos][D/2][2] (cos, sin)
  const int* pos;       // [B]
};

template <int D, int G, int VAR>
__global__ void __launch_bounds__(256)
decode_attn_kernel(const bf16_t* __restrict__ q, int ldq, const bf16_t* __restrict__ kc,
                   const bf16_t* __restrict__ vc, const int* __restrict__ lens, const int* __restrict__ slot,
                   const int* __restrict__ pre,
                   int H, int Hkv, int max_seq, int chunk_max, int nsplit, float scale_log2e,
                   float* __restrict__ po, float* __restrict__ pm, float* __restrict__ pl,
                   bf16_t* __restrict__ out, int ldo, int* __restrict__ cnt, DecRope rope) {
  constexpr int KT = 64;
  constexpr int CPR = D / 8;                       // 16-B chunks per key row
  constexpr int GCD = (CPR % 16 == 0) ? 16 : ((CPR % 8 == 0) ? 8 : ((CPR % 4 == 0) ? 4 : 2));
  constexpr int NSET = CPR / GCD;                  // distinct dim-slots per lane
  constexpr bool SHFL = (64 % CPR) == 0;           // a key's chunks live in one wave-instruction
  // 4 waves per workgroup (8, a split's tiles all in flight at once at batch 1, measured 2x slower:
  // profiles/r4/rejected_r4.txt)
  constexpr int NWV = 4, NTH = 64 * NWV;
  __shared__ float sq[G][D];
  __shared__ float sp[NWV][G][KT];
  __shared__ float spart[SHFL ? 1 : NWV][SHFL ? 1 : G * KT * CPR];
  __shared__ float so[G == 1 ? 1 : NWV][G][D];
  __shared__ float sacc[G == 1 ? NWV * NSET * 64 * 8 : 1];
  __shared__ float swm[NWV][G], swl[NWV][G];

  // VAR bit3 (XC): workgroup w of the launch runs on XCD w % 8 (round-robin dispatch; the host
  // enables XC only after a placement probe confirmed it), so (b, kv head) pair p takes the nsplit
  // workgroups w = 8 * (nsplit * (p / 8) + split) + p % 8: all of its splits on one XCD, their
  // partials exchanged through that XCD's L2 (dec_finish<XC>). Needs (B * Hkv) % 8 == 0.
  constexpr bool XC = (VAR & DEC_XC) != 0;
  int split = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
  if constexpr (XC) {
    const int wl = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
    const int s8 = wl >> 3, pair = (s8 / nsplit) * 8 + (wl & 7);
    split = s8 % nsplit;
    hk = pair % Hkv;
    b = pair / Hkv;
  }
  const int L = lens[b];
  DA_ASSERT(L >= 0 && L <= max_seq && slot[b] >= 0);
  const int chunk = dec_chunk(L, nsplit, chunk_max);
  const int kstart = split * chunk;
  const bool fr = rope.cs != nullptr;
  const bool own_new = fr && kstart <= L - 1 && L - 1 < kstart + chunk;  // this split holds key L-1
  const int kend = min(fr ? L - 1 : L, kstart + chunk);                  // fused: key L-1 comes from qkv
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const size_t cbase = ((size_t)slot[b] * Hkv + hk) * (size_t)max_seq * D;
  const int P = pre ? pre[2 * b] : 0;  // shared-prefix keys [0, P) live in slot pre[2b + 1]
  const size_t pbase = P ? ((size_t)pre[2 * b + 1] * Hkv + hk) * (size_t)max_seq * D : cbase;
  DA_ASSERT(P >= 0 && P <= L);
  DA_ASSERT(!fr || rope.pos[b] == L - 1);
  __shared__ float skn[D], svn[D], ssn[G];

  // VAR bit0: non-temporal loads (the KV stream is read once per step); bit1: V issued together
  // with K (else after the scores: ~100 VGPRs live instead of ~200, so 4-5 waves per SIMD hide the
  // HBM latency instead of 2); bit2 (small batches, implies bit1): the wave's NEXT tile is loaded
  // before the current one is computed — at batch 1 a workgroup's few tiles are latency-bound, one
  // HBM round trip each, and occupancy buys nothing. Loads are branch-free (chunk index clamped
  // into the tile; keys >= nk get p = 0) so the compiler's vmcnt waits stay counted.
  constexpr bool NT = (VAR & DEC_NT) != 0, PFT = (VAR & DEC_PFT) != 0, VEARLY = PFT || (VAR & DEC_VEARLY) != 0;
  auto ld16 = [&](const bf16_t* p) -> u32x4_t {
    if constexpr (NT) return __builtin_nontemporal_load((const u32x4_t*)p);
    else return *(const u32x4_t*)p;
  };
  auto tile_base = [&](const bf16_t* c, int t0) {
    return c + (t0 < P ? pbase : cbase) + (size_t)t0 * D;
  };
  // PFT loads are branch-free: a tile past kend reads key 0 of the row's own slot (one line, valid
  // memory, never used) so the prefetches can be issued unconditionally.
  // The tile that holds key P when P is no multiple of 64 takes its keys below P from the prefix slot
  // and the others from the row's own: per-lane select in the PFT form (no branch around its loads),
  // a wave-uniform branch otherwise, so that whole-tile prefixes run the loads they always ran.
  auto load_kv = [&](const bf16_t* c, u32x4_t (&x)[CPR], int t0) {
    const int nk = kend - t0;
    const int last = min(KT, nk) * CPR - 1;
    const bf16_t* tb = tile_base(c, t0);
    const bf16_t* to = c + cbase + (size_t)t0 * D;                    // the same tile of the row's own slot
    const bool str = t0 < P && P < t0 + KT;
    const int cut = str ? (P - t0) * CPR : KT * CPR;                  // chunks below it: the tile's own source
    if constexpr (PFT) {
#pragma unroll
      for (int i = 0; i < CPR; ++i) {
        const int cc = min(i * 64 + lane, last);
        x[i] = ld16(nk > 0 ? (cc < cut ? tb : to) + cc * 8 : c + cbase);
      }
    } else if (str) {
#pragma unroll
      for (int i = 0; i < CPR; ++i) {
        const int cc = i * 64 + lane;
        x[i] = (cc <= last) ? ld16((cc < cut ? tb : to) + cc * 8) : u32x4_t{0, 0, 0, 0};
      }
    } else {
#pragma unroll
      for (int i = 0; i < CPR; ++i) {
        const int cc = i * 64 + lane;
        x[i] = (cc <= last) ? ld16(tb + cc * 8) : u32x4_t{0, 0, 0, 0};
      }
    }
  };
  auto load_k = [&](u32x4_t (&kv)[CPR], int t0) { load_kv(kc, kv, t0); };
  auto load_v = [&](u32x4_t (&vv)[CPR], int t0) { load_kv(vc, vv, t0); };
  // RoPE (interleaved pairs (2i, 2i+1)) of one element of a head row, rounded to bf16 like the
  // rope_cache kernel / the QKV GEMM epilogue that this path replaces
  constexpr int HALF = D / 2;
  auto rot2 = [&](float x1, float x2, float c, float sn, int d) -> float {
    return bf2f(f2bf((d & 1) ? x2 * c + x1 * sn : x1 * c - x2 * sn));
  };
  auto rot = [&](const bf16_t* hp, int d, int p) -> float {
    const int i = d >> 1;
    return rot2(bf2f(hp[d & ~1]), bf2f(hp[d | 1]), rope.cs[((size_t)p * HALF + i) * 2],
                rope.cs[((size_t)p * HALF + i) * 2 + 1], d);
  };
  // PFT (small batches): the prologue's operands (this thread's q element, its RoPE partner and
  // cos / sin, the new token's k / v element) are loaded FIRST, then the first two K/V tiles of the
  // wave are requested, unconditionally (an empty tile reads one line), so the compiler's counted
  // wait for the prologue leaves the K/V stream in flight: its first HBM round trip overlaps the
  // prologue instead of following it (vmcnt retires loads in order).
  constexpr bool PRE = PFT && G * D <= 256;
  u32x4_t ka[PFT ? CPR : 1], va[PFT ? CPR : 1], kb2[PFT ? CPR : 1], vb2[PFT ? CPR : 1];
  if constexpr (PRE) {
    // straight-line, clamped loads of raw bits: no branch and no use before the K/V loads below, so
    // the wait for them is a counted vmcnt(48), not vmcnt(0) (a use inside a branch forces the latter)
    const int qi = min(tid, G * D - 1), d = qi % D;
    const bf16_t* hp = q + (size_t)b * ldq + (hk * G + qi / D) * D;
    const bf16_t rq1 = hp[d & ~1], rq2 = hp[d | 1];
    const float* csp = fr ? rope.cs + ((size_t)(L - 1) * HALF + (d >> 1)) * 2 : (const float*)hp;
    const f32x2_t rcs = *(const f32x2_t*)csp;
    const bf16_t* kr = fr ? q + (size_t)b * ldq + (size_t)(H + hk) * D : hp;
    const bf16_t* vr = fr ? q + (size_t)b * ldq + (size_t)(H + Hkv + hk) * D : hp;
    const bf16_t rk1 = kr[d & ~1], rk2 = kr[d | 1], nv = vr[d];
    const int t0 = kstart + w * KT, t1 = t0 + NWV * KT;
    load_k(ka, t0); load_v(va, t0);
    load_k(kb2, t1); load_v(vb2, t1);
    const float pc = fr ? rcs[0] : 1.f, ps = fr ? rcs[1] : 0.f;
    if (tid < G * D) {
      const float px1 = bf2f(rq1), px2 = bf2f(rq2);
      const float x = fr ? rot2(px1, px2, pc, ps, d) : ((d & 1) ? px2 : px1);
      sq[tid / D][d] = x * scale_log2e;
    }
    if (own_new && tid < D) {
      const size_t crow = cbase + (size_t)(L - 1) * D;
      const float kv = rot2(bf2f(rk1), bf2f(rk2), pc, ps, d);  // same position L - 1 -> same cos / sin
      skn[d] = kv;
      svn[d] = bf2f(nv);
      rope.kc[crow + d] = f2bf(kv);  // for later steps (read back only after this launch)
      rope.vc[crow + d] = nv;
    }
  } else {
    if constexpr (PFT) {
      const int t0 = kstart + w * KT, t1 = t0 + NWV * KT;
      load_k(ka, t0); load_v(va, t0);
      load_k(kb2, t1); load_v(vb2, t1);
    }
    for (int i = tid; i < G * D; i += NTH) {
      const int g = i / D, d = i % D;
      const bf16_t* hp = q + (size_t)b * ldq + (hk * G + g) * D;
      sq[g][d] = (fr ? rot(hp, d, L - 1) : bf2f(hp[d])) * scale_log2e;
    }
  }
  if (own_new && !PRE) {
    const size_t crow = cbase + (size_t)(L - 1) * D;
    const bf16_t* kr = q + (size_t)b * ldq + (size_t)(H + hk) * D;
    const bf16_t* vr = q + (size_t)b * ldq + (size_t)(H + Hkv + hk) * D;
    for (int d = tid; d < D; d += NTH) {
      const float kv = rot(kr, d, L - 1);
      skn[d] = kv;
      svn[d] = bf2f(vr[d]);
      rope.kc[crow + d] = f2bf(kv);  // for later steps (read back only after this launch)
      rope.vc[crow + d] = vr[d];
    }
  }
  if constexpr (G > 1) {
    for (int i = tid; i < NWV * G * D; i += NTH) (&so[0][0][0])[i] = 0.f;
  }
  __syncthreads();
  if (own_new && w == 0) {  // score of the new key for each query head of this kv head
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float part = 0.f;
      for (int d = lane; d < D; d += 64) part += sq[g][d] * skn[d];
      part = wave_sum(part);
      if (lane == 0) ssn[g] = part;
    }
  }

  float m[G], l[G], acc[G][NSET][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    m[g] = -INFINITY; l[g] = 0.f;
#pragma unroll
    for (int s = 0; s < NSET; ++s)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[g][s][e] = 0.f;
  }

  auto process = [&](const u32x4_t (&kv)[CPR], u32x4_t (&vv)[CPR], int t0) {
    const int nk = min(KT, kend - t0);
    // ---- scores ----
#pragma unroll
    for (int i = 0; i < CPR; ++i) {
      const int c = i * 64 + lane;
      const int dp = c % CPR;
      float kf[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        kf[2 * e] = bf2f((bf16_t)(kv[i][e] & 0xffff));
        kf[2 * e + 1] = bf2f((bf16_t)(kv[i][e] >> 16));
      }
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const f32x4_t q0 = *(const f32x4_t*)&sq[g][dp * 8];
        const f32x4_t q1 = *(const f32x4_t*)&sq[g][dp * 8 + 4];
        float part = kf[0] * q0[0] + kf[1] * q0[1] + kf[2] * q0[2] + kf[3] * q0[3] +
                     kf[4] * q1[0] + kf[5] * q1[1] + kf[6] * q1[2] + kf[7] * q1[3];
        if constexpr (SHFL) {
#pragma unroll
          for (int o = 1; o < CPR; o <<= 1) part += __shfl_xor(part, o, 64);
          if (dp == 0) sp[w][g][c / CPR] = part;
        } else {
          spart[w][g * KT * CPR + c] = part;
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // ---- online softmax; lane = key ----
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float sc;
      if constexpr (SHFL) {
        sc = sp[w][g][lane];
      } else {
        sc = 0.f;
#pragma unroll
        for (int j = 0; j < CPR; ++j) sc += spart[w][g * KT * CPR + lane * CPR + j];
      }
      if (lane >= nk) sc = -INFINITY;
      const float tmax = wave_max(sc);
      const float m_new = fmaxf(m[g], tmax);
      const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
      const float alpha = exp2f(m[g] - m_use);
      const float p = exp2f(sc - m_use);
      l[g] = l[g] * alpha + wave_sum(p);
      m[g] = m_new;
      sp[w][g][lane] = p;
#pragma unroll
      for (int st = 0; st < NSET; ++st)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[g][st][e] *= alpha;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // ---- P * V ----
    asm volatile("" ::: "memory");
    if constexpr (!VEARLY) load_v(vv, t0);
#pragma unroll
    for (int i = 0; i < CPR; ++i) {
      const int c = i * 64 + lane;
      const int key = c / CPR;
      float vf[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        vf[2 * e] = bf2f((bf16_t)(vv[i][e] & 0xffff));
        vf[2 * e + 1] = bf2f((bf16_t)(vv[i][e] >> 16));
      }
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float pk = sp[w][g][key];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[g][i % NSET][e] += pk * vf[e];
      }
    }
    __builtin_amdgcn_wave_barrier();
  };

  if constexpr (PFT) {  // two tiles in flight per wave: ka/va and kb2/vb2 alternate
    int t0 = kstart + w * KT;
    while (t0 < kend) {
      const int t1 = t0 + NWV * KT;
      process(ka, va, t0);
      if (t1 >= kend) break;
      const int t2 = t1 + NWV * KT;
      if (t2 < kend) { load_k(ka, t2); load_v(va, t2); }
      process(kb2, vb2, t1);
      if (t2 >= kend) break;
      const int t3 = t2 + NWV * KT;
      if (t3 < kend) { load_k(kb2, t3); load_v(vb2, t3); }
      t0 = t2;
    }
  } else {
    for (int t0 = kstart + w * KT; t0 < kend; t0 += NWV * KT) {
      u32x4_t kv[CPR], vv[CPR];
      load_k(kv, t0);
      if constexpr (VEARLY) load_v(vv, t0);
      process(kv, vv, t0);
    }
  }
  // ---- merge lanes -> per-wave O, then waves -> block partial ----
  // MHA (G = 1): every lane parks its accumulators in LDS with plain 16-B stores and the output
  // threads sum the (dim-slot, lane) entries that hold their dim. LDS float atomics — 5-6 lanes per
  // address — took 7.5 us of a 20 us batch-1 launch (bench/decode_trace.py), more than the K/V stream.
  if constexpr (G == 1) {
#pragma unroll
    for (int st = 0; st < NSET; ++st) {
      float* dst = &sacc[((w * NSET + st) * 64 + lane) * 8];
      *(f32x4_t*)dst = f32x4_t{acc[0][st][0], acc[0][st][1], acc[0][st][2], acc[0][st][3]};
      *(f32x4_t*)(dst + 4) = f32x4_t{acc[0][st][4], acc[0][st][5], acc[0][st][6], acc[0][st][7]};
    }
  } else {
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int st = 0; st < NSET; ++st) {
        const int dp = (lane + 64 * st) % CPR;
#pragma unroll
        for (int e = 0; e < 8; ++e) atomicAdd(&so[w][g][dp * 8 + e], acc[g][st][e]);
      }
  }
  if (lane == 0) {
#pragma unroll
    for (int g = 0; g < G; ++g) { swm[w][g] = m[g]; swl[w][g] = l[g]; }
  }
  __syncthreads();
  for (int i = tid; i < G * D; i += NTH) {
    const int g = i / D, d = i % D;
    float M = fmaxf(fmaxf(swm[0][g], swm[1][g]), fmaxf(swm[2][g], swm[3][g]));
#pragma unroll
    for (int ww = 4; ww < NWV; ++ww) M = fmaxf(M, swm[ww][g]);
    if (own_new) M = fmaxf(M, ssn[g]);
    const float Mu = (M == -INFINITY) ? 0.f : M;
    float o = 0.f, ls = 0.f;
#pragma unroll
    for (int ww = 0; ww < NWV; ++ww) {
      const float f = exp2f(swm[ww][g] - Mu);
      float ow;
      if constexpr (G == 1) {
        // lane l's slot st holds dims 8 * ((64 st + l) % CPR) .. +7
        // fixed trip counts: all of a wave's reads are independent and issued back to back
        ow = 0.f;
        const int dp = d >> 3, e = d & 7;
#pragma unroll
        for (int st = 0; st < NSET; ++st) {
          const int l0 = ((dp - 64 * st) % CPR + CPR) % CPR;
#pragma unroll
          for (int j = 0; j < (64 + CPR - 1) / CPR; ++j) {
            const int l = l0 + j * CPR;
            if (l < 64) ow += sacc[((ww * NSET + st) * 64 + l) * 8 + e];
          }
        }
      } else {
        ow = so[ww][g][d];
      }
      o += ow * f;
      ls += swl[ww][g] * f;
    }
    if (own_new) {  // the new token's key: weight exp2(s - M), value straight from the qkv row
      const float f = exp2f(ssn[g] - Mu);
      o += svn[d] * f;
      ls += f;
    }
    dec_store(o, M, ls, b, hk * G + g, d, H, nsplit, split, D, po, pm, pl, out, ldo);
  }
  __shared__ int s_last;
  dec_finish<D, G, XC>(po, pm, pl, H, Hkv, nsplit, b, hk, cnt, out, ldo, &s_last);
}

// ------------------------------------------------------------------------------------------
// GQA decode attention on MFMA (G = H/Hkv query heads share one KV head: Llama-3-8B G=4,
// Llama-3-70B at TP=8 G=8). The G queries of a KV head form the N=16 side of
// v_mfma_f32_16x16x32_bf16 (zero-padded), so K and V are read once per KV head instead of being
// multiplied against each query on the VALU (the G >= 2 path of decode_attn_kernel is VALU-bound).
// Per wave and 64-key tile:
//   S^T[key][g] = K·Q^T : A = K rows straight from HBM into registers (non-temporal 16-B loads),
//                         B = Q^T (registers, loaded once);
//   softmax over the 64 keys of each query column: 16 values per lane + two cross-lane steps;
//   O^T[d][g] += V^T·P^T : B = P^T from the S^T registers (k index permuted), A = V^T read from the
//                         wave's private LDS copy of the V tile with ds_read_b64_tr_b16. The V tile
//                         is a contiguous [64 x D] block of the cache, so it is copied by LDS-DMA
//                         (global_load_lds, 1 KiB per wave-instruction) with an XOR chunk swizzle
//                         on the source address that makes the transposed reads conflict-free.
template <int D>
__device__ __forceinline__ int vswz(int r) {
  return D == 128 ? ((r & 7) << 1) : (((r >> 1) & 3) << 1);
}

template <int D, int G>
__global__ void __launch_bounds__(256)
decode_attn_gqa_kernel(const bf16_t* __restrict__ q, int ldq, const bf16_t* __restrict__ kc,
                       const bf16_t* __restrict__ vc, const int* __restrict__ lens, const int* __restrict__ slot,
                   const int* __restrict__ pre,
                       int H, int Hkv, int max_seq, int chunk_max, int nsplit, float scale_log2e,
                       float* __restrict__ po, float* __restrict__ pm, float* __restrict__ pl,
                       bf16_t* __restrict__ out, int ldo, int* __restrict__ cnt) {
  static_assert(D == 64 || D == 128, "GQA MFMA decode supports head dims 64 and 128");
  constexpr int KT = 64, NDS = D / 32, NDT = D / 16, NS = D / 8;   // d-steps (S), d-tiles (O), 16-B chunks/row
  constexpr int VBYTES = KT * D * 2, NDMA = VBYTES / 1024;
  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  typedef __attribute__((address_space(1))) const void* gptr_t;
  __shared__ __attribute__((aligned(16))) char sv[4 * VBYTES];
  __shared__ float swm[4][16], swl[4][16];

  const int split = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
  const int L = lens[b];
  DA_ASSERT(L >= 0 && L <= max_seq && slot[b] >= 0);
  const int chunk = dec_chunk(L, nsplit, chunk_max);
  const int kstart = split * chunk;
  const int kend = min(L, kstart + chunk);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const size_t cbase = ((size_t)slot[b] * Hkv + hk) * (size_t)max_seq * D;
  const int P = pre ? pre[2 * b] : 0;  // shared-prefix keys [0, P) live in slot pre[2b + 1]
  const size_t pbase = P ? ((size_t)pre[2 * b + 1] * Hkv + hk) * (size_t)max_seq * D : cbase;
  DA_ASSERT(P >= 0 && P <= L);
  char* myv = sv + w * VBYTES;

  bf16x8_t qf[NDS];
#pragma unroll
  for (int ds = 0; ds < NDS; ++ds) {
    if (fr < G) qf[ds] = *(const bf16x8_t*)(q + (size_t)b * ldq + (hk * G + fr) * D + ds * 32 + fg * 8);
    else qf[ds] = bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0};
  }
  f32x4_t oacc[NDT];
#pragma unroll
  for (int i = 0; i < NDT; ++i) oacc[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_part = 0.f;

  for (int t0 = kstart + w * KT; t0 < kend; t0 += 4 * KT) {
    const int nk = min(KT, kend - t0);
    const bool shared = t0 < P;
    const bf16_t* kb = kc + (shared ? pbase : cbase) + (size_t)t0 * D;
    const bf16_t* vb = vc + (shared ? pbase : cbase) + (size_t)t0 * D;
    // ---- K straight to registers (A operand rows = keys), then the V tile by LDS-DMA ----
    // STR: the tile that holds key P when P is no multiple of 64 — its keys from P on come from the
    // row's own slot (a wave-uniform branch: whole-tile prefixes run the loads they always ran)
    u32x4_t kr[4][NDS];
    auto issue = [&](auto STR) {
      constexpr bool S = decltype(STR)::value;
      [[maybe_unused]] const int npre = P - t0;
      [[maybe_unused]] const bf16_t* ko = kc + cbase + (size_t)t0 * D;
      [[maybe_unused]] const bf16_t* vo = vc + cbase + (size_t)t0 * D;
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int ds = 0; ds < NDS; ++ds) {
          const int key = min(16 * t + fr, nk - 1);
          const bf16_t* base = (S && key >= npre) ? ko : kb;
          const u32x4_t* src = (const u32x4_t*)(base + (size_t)key * D + ds * 32 + fg * 8);
          kr[t][ds] = __builtin_nontemporal_load(src);
        }
#pragma unroll
      for (int i = 0; i < NDMA; ++i) {
        const int pc = i * 64 + lane, row = pc / NS, sl = pc % NS;
        const int c = sl ^ vswz<D>(row);
        const int key = min(row, nk - 1);
        const bf16_t* base = (S && key >= npre) ? vo : vb;
        // aux 2 = nt (read once per step; see decode_attn_mfma1_kernel)
        __builtin_amdgcn_global_load_lds((gptr_t)(base + (size_t)key * D + c * 8), (lds_ptr_t)(myv + i * 1024), 16, 0, 2);
      }
    };
    if (shared && P < t0 + KT) issue(std::true_type{});
    else issue(std::false_type{});
    // ---- S^T = K Q^T ----
    f32x4_t sacc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      sacc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ds = 0; ds < NDS; ++ds) sacc[t] = mfma16(__builtin_bit_cast(bf16x8_t, kr[t][ds]), qf[ds], sacc[t]);
    }
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = 16 * t + 4 * fg + i;
        const float sc = key < nk ? sacc[t][i] * scale_log2e : -INFINITY;
        sacc[t][i] = sc;
        mx = fmaxf(mx, sc);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = max_xhalf(mx);
    const float m_new = fmaxf(m_run, mx);
    const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
    const float alpha = exp2f(m_run - m_use);
    m_run = m_new;
    float psum = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float p = __builtin_amdgcn_exp2f(sacc[t][i] - m_use);
        sacc[t][i] = p;
        psum += p;
      }
    l_part = l_part * alpha + psum;
#pragma unroll
    for (int i = 0; i < NDT; ++i) oacc[i] *= alpha;
    // ---- O^T += V^T P^T: k-step c covers keys 32c..32c+31; slot j -> key 32c + 16(j>>2) + 4fg + (j&3) ----
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's V DMA landed (wave-private LDS)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const u32x4_t pw = u32x4_t{pack_bf2(sacc[2 * c][0], sacc[2 * c][1]), pack_bf2(sacc[2 * c][2], sacc[2 * c][3]),
                                 pack_bf2(sacc[2 * c + 1][0], sacc[2 * c + 1][1]),
                                 pack_bf2(sacc[2 * c + 1][2], sacc[2 * c + 1][3])};
      const bf16x8_t pb = __builtin_bit_cast(bf16x8_t, pw);
      const int q4 = fr >> 2, p4 = fr & 3;
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        const int col = dt * 16 + 4 * p4;                      // 4 columns of this lane's address
        const int r0 = 32 * c + 4 * fg + q4, r1 = r0 + 16;
        const s16x4_t lo = lds_read_tr16(myv + r0 * (D * 2) + (((col >> 3) ^ vswz<D>(r0)) << 4) + (col & 7) * 2);
        const s16x4_t hi = lds_read_tr16(myv + r1 * (D * 2) + (((col >> 3) ^ vswz<D>(r1)) << 4) + (col & 7) * 2);
        const bf16x8_t va = bf16x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        oacc[dt] = mfma16(va, pb, oacc[dt]);
      }
    }
    // the next tile's DMA rewrites this wave's V region: finish the tr-reads first
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
  // ---- merge the 4 waves: per-query (m, l) and O^T partials through LDS ----
  float l_tot = l_part + __shfl_xor(l_part, 16, 64);
  l_tot = sum_xhalf(l_tot);
  if (fg == 0) { swm[w][fr] = m_run; swl[w][fr] = l_tot; }
  __syncthreads();  // every wave is done with its V region
  float* so = (float*)sv;  // [4][16][D]
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
    for (int i = 0; i < 4; ++i) so[(w * 16 + fr) * D + dt * 16 + 4 * fg + i] = oacc[dt][i];
  __syncthreads();
  for (int i = tid; i < G * D; i += 256) {
    const int g = i / D, d = i % D;
    const float M = fmaxf(fmaxf(swm[0][g], swm[1][g]), fmaxf(swm[2][g], swm[3][g]));
    const float Mu = (M == -INFINITY) ? 0.f : M;
    float o = 0.f, ls = 0.f;
#pragma unroll
    for (int ww = 0; ww < 4; ++ww) {
      const float f = exp2f(swm[ww][g] - Mu);
      o += so[(ww * 16 + g) * D + d] * f;
      ls += swl[ww][g] * f;
    }
    dec_store(o, M, ls, b, hk * G + g, d, H, nsplit, split, D, po, pm, pl, out, ldo);
  }
  __shared__ int s_last;
  dec_finish<D, G>(po, pm, pl, H, Hkv, nsplit, b, hk, cnt, out, ldo, &s_last);
}

// MHA decode attention on MFMA for few (row, kv head) pairs (batch 1..: the p50 path). The VALU
// kernel (decode_attn_kernel, G = 1) spends ~2k VALU cycles per 64-key tile on its dot products, so
// at batch 1 — 32 pairs, a few tiles per wave — it is issue-bound, not HBM-bound (profiles/r5/
// decode_mfma1/: 2.9 TB/s even with the K/V in the MALL). Here the single query is the N = 16 side of
// v_mfma_f32_16x16x32_bf16 (column 0 live, 15 zero), exactly the GQA kernel's data path with G = 1:
// K rows straight into registers (non-temporal), the V tile by LDS-DMA into a wave-private region
// (XOR chunk swizzle within groups of 4 chunks, so D = 96's 12 chunks per row stay in the row),
// S^T = K Q^T, softmax over column 0, O^T += V^T P^T with transposed LDS reads. chunk <= 512 keys per
// split (host-checked) gives every wave at most TWO tiles, and both are requested before any is
// waited for: one HBM round trip per workgroup. XC: same-XCD split exchange (see dec_finish).
template <int D>
__device__ __forceinline__ int vswz1(int r) {
  return D == 96 ? ((r >> 1) & 3) : vswz<D>(r);
}

// RP: fused RoPE + new-token KV write (DecRope, as decode_attn_kernel): q is the raw qkv row; q is
// rotated into LDS while the tiles fly, key L - 1 enters as one extra online-softmax term of the
// split that holds it (taken from the qkv row, written into the cache for later steps).
template <int D, bool XC, bool RP>
__global__ void __launch_bounds__(256)
decode_attn_mfma1_kernel(const bf16_t* __restrict__ q, int ldq, const bf16_t* __restrict__ kc,
                         const bf16_t* __restrict__ vc, const int* __restrict__ lens, const int* __restrict__ slot,
                         const int* __restrict__ pre, int H, int Hkv, int max_seq, int chunk_max, int nsplit,
                         float scale_log2e, float* __restrict__ po, float* __restrict__ pm, float* __restrict__ pl,
                         bf16_t* __restrict__ out, int ldo, int* __restrict__ cnt, DecRope rope) {
  static_assert(D == 64 || D == 96 || D == 128, "head dim");
  constexpr int KT = 64, NDS = D / 32, NDT = D / 16, NS = D / 8;
  constexpr int VBYTES = KT * D * 2, NDMA = VBYTES / 1024;
  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  typedef __attribute__((address_space(1))) const void* gptr_t;
  __shared__ __attribute__((aligned(16))) char sv[4 * 2 * VBYTES];  // two tiles per wave
  __shared__ float swm[4], swl[4];

  int split = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
  if constexpr (XC) {  // the same-XCD mapping of decode_attn_kernel
    const int wl = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
    const int s8 = wl >> 3, pair = (s8 / nsplit) * 8 + (wl & 7);
    split = s8 % nsplit;
    hk = pair % Hkv;
    b = pair / Hkv;
  }
  const int L = lens[b];
  DA_ASSERT(L >= 0 && L <= max_seq && slot[b] >= 0);
  const int chunk = dec_chunk(L, nsplit, chunk_max);
  DA_ASSERT(chunk <= 8 * KT);
  const int kstart = split * chunk;
  const bool own_new = RP && kstart <= L - 1 && L - 1 < kstart + chunk;  // this split holds key L - 1
  const int kend = min(RP ? L - 1 : L, kstart + chunk);                  // RP: key L - 1 from the qkv row
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const size_t cbase = ((size_t)slot[b] * Hkv + hk) * (size_t)max_seq * D;
  const int P = pre ? pre[2 * b] : 0;  // shared-prefix keys [0, P) live in slot pre[2b + 1]
  const size_t pbase = P ? ((size_t)pre[2 * b + 1] * Hkv + hk) * (size_t)max_seq * D : cbase;
  DA_ASSERT(P >= 0 && P <= L);
  DA_ASSERT(!RP || rope.pos[b] == L - 1);

  // ---- both tiles of this wave requested up front (branch-free: an empty tile reads key 0 of
  //      the row's own slot, valid memory whose scores are masked) ----
  const int ta = kstart + w * KT, tb = ta + 4 * KT;
  u32x4_t kr[2][4][NDS];
  // STR: the tile that holds key P when P is no multiple of 64 — its keys from P on come from the
  // row's own slot (a wave-uniform branch in issue(): whole-tile prefixes run the loads they always ran)
  auto issue_tile = [&](auto STR, int j, int t0) {
    constexpr bool S = decltype(STR)::value;
    const int nk = kend - t0;
    const bool shared = t0 < P;
    const bf16_t* kb = nk > 0 ? kc + (shared ? pbase : cbase) + (size_t)t0 * D : kc + cbase;
    const bf16_t* vb = nk > 0 ? vc + (shared ? pbase : cbase) + (size_t)t0 * D : vc + cbase;
    const int last = nk > 0 ? min(KT, nk) - 1 : 0;
    [[maybe_unused]] const int npre = P - t0;  // S: nk > 0 (issue() checks), so kb / vb are the prefix slot's tile
    [[maybe_unused]] const bf16_t* ko = kc + cbase + (size_t)t0 * D;
    [[maybe_unused]] const bf16_t* vo = vc + cbase + (size_t)t0 * D;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int ds = 0; ds < NDS; ++ds) {
        const int key = min(16 * t + fr, last);
        const bf16_t* base = (S && key >= npre) ? ko : kb;
        kr[j][t][ds] = __builtin_nontemporal_load((const u32x4_t*)(base + (size_t)key * D + ds * 32 + fg * 8));
      }
    char* myv = sv + (w * 2 + j) * VBYTES;
#pragma unroll
    for (int i = 0; i < NDMA; ++i) {
      const int pc = i * 64 + lane, row = pc / NS, sl = pc % NS;
      const int c = sl ^ vswz1<D>(row);
      const int key = min(row, last);
      const bf16_t* base = (S && key >= npre) ? vo : vb;
      // aux 2 = nt: the KV stream is read once per step; allocating it in L2 / MALL cost the GEMVs
      // that follow ~3 % (their weights lose cache residency): profiles/r5/decode_mfma1/
      __builtin_amdgcn_global_load_lds((gptr_t)(base + (size_t)key * D + c * 8), (lds_ptr_t)(myv + i * 1024), 16, 0, 2);
    }
  };
  auto issue = [&](int j, int t0) {
    if (t0 < P && P < t0 + KT && t0 < kend) issue_tile(std::true_type{}, j, t0);
    else issue_tile(std::false_type{}, j, t0);
  };
  issue(0, ta);
  issue(1, tb);

  bf16x8_t qf[NDS];
  [[maybe_unused]] __shared__ __attribute__((aligned(16))) bf16_t sqb[RP ? D : 1];
  [[maybe_unused]] __shared__ float skn[RP ? D : 1], svn[RP ? D : 1];
  [[maybe_unused]] __shared__ float ssn;
  if constexpr (RP) {
    // rotate q (and the new key) at position L - 1, rounded to bf16 like the rope_cache kernel
    constexpr int HALF = D / 2;
    const bf16_t* qrow = q + (size_t)b * ldq;
    if (tid < D) {
      const int d = tid, i = d >> 1;
      const float c = rope.cs[((size_t)(L - 1) * HALF + i) * 2], sn = rope.cs[((size_t)(L - 1) * HALF + i) * 2 + 1];
      auto rot = [&](const bf16_t* hp) {
        const float x1 = bf2f(hp[d & ~1]), x2 = bf2f(hp[d | 1]);
        return f2bf((d & 1) ? x2 * c + x1 * sn : x1 * c - x2 * sn);
      };
      sqb[d] = rot(qrow + hk * D);
      if (own_new) {
        const bf16_t kn = rot(qrow + (size_t)(H + hk) * D), vn = qrow[(size_t)(H + Hkv + hk) * D + d];
        skn[d] = bf2f(kn);
        svn[d] = bf2f(vn);
        const size_t crow = cbase + (size_t)(L - 1) * D;
        rope.kc[crow + d] = kn;  // for later steps (read back only after this launch)
        rope.vc[crow + d] = vn;
      }
    }
    __syncthreads();
#pragma unroll
    for (int ds = 0; ds < NDS; ++ds)
      qf[ds] = fr == 0 ? *(const bf16x8_t*)(sqb + ds * 32 + fg * 8) : bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0};
    if (own_new && w == 0) {  // score of the new key (log2 units)
      float part = 0.f;
      for (int d = lane; d < D; d += 64) part += bf2f(sqb[d]) * skn[d];
      part = wave_sum(part);
      if (lane == 0) ssn = part * scale_log2e;
    }
  } else {
#pragma unroll
    for (int ds = 0; ds < NDS; ++ds)
      qf[ds] = fr == 0 ? *(const bf16x8_t*)(q + (size_t)b * ldq + hk * D + ds * 32 + fg * 8)
                       : bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0};
  }
  f32x4_t oacc[NDT];
#pragma unroll
  for (int i = 0; i < NDT; ++i) oacc[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_part = 0.f;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // both tiles' K registers and V regions landed

  auto process = [&](int j, int t0) {
    const int nk = kend - t0;
    f32x4_t sacc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      sacc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ds = 0; ds < NDS; ++ds) sacc[t] = mfma16(__builtin_bit_cast(bf16x8_t, kr[j][t][ds]), qf[ds], sacc[t]);
    }
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = 16 * t + 4 * fg + i;
        const float sc = key < nk ? sacc[t][i] * scale_log2e : -INFINITY;
        sacc[t][i] = sc;
        mx = fmaxf(mx, sc);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = max_xhalf(mx);
    const float m_new = fmaxf(m_run, mx);
    const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
    const float alpha = exp2f(m_run - m_use);
    m_run = m_new;
    float psum = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float p = __builtin_amdgcn_exp2f(sacc[t][i] - m_use);
        sacc[t][i] = p;
        psum += p;
      }
    l_part = l_part * alpha + psum;
#pragma unroll
    for (int i = 0; i < NDT; ++i) oacc[i] *= alpha;
    const char* myv = sv + (w * 2 + j) * VBYTES;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const u32x4_t pw = u32x4_t{pack_bf2(sacc[2 * c][0], sacc[2 * c][1]), pack_bf2(sacc[2 * c][2], sacc[2 * c][3]),
                                 pack_bf2(sacc[2 * c + 1][0], sacc[2 * c + 1][1]),
                                 pack_bf2(sacc[2 * c + 1][2], sacc[2 * c + 1][3])};
      const bf16x8_t pb = __builtin_bit_cast(bf16x8_t, pw);
      const int q4 = fr >> 2, p4 = fr & 3;
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        const int col = dt * 16 + 4 * p4;
        const int r0 = 32 * c + 4 * fg + q4, r1 = r0 + 16;
        const s16x4_t lo = lds_read_tr16(myv + r0 * (D * 2) + (((col >> 3) ^ vswz1<D>(r0)) << 4) + (col & 7) * 2);
        const s16x4_t hi = lds_read_tr16(myv + r1 * (D * 2) + (((col >> 3) ^ vswz1<D>(r1)) << 4) + (col & 7) * 2);
        const bf16x8_t va = bf16x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        oacc[dt] = mfma16(va, pb, oacc[dt]);
      }
    }
  };
  if (ta < kend) process(0, ta);
  if (tb < kend) process(1, tb);

  // ---- merge the 4 waves (query column 0: lanes fr == 0) through LDS ----
  float l_tot = l_part + __shfl_xor(l_part, 16, 64);
  l_tot = sum_xhalf(l_tot);
  if (lane == 0) { swm[w] = m_run; swl[w] = l_tot; }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();  // every wave is done with its V regions
  float* so = (float*)sv;  // [4][D]: column 0 of each wave's O^T
  if (fr == 0) {
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
      for (int i = 0; i < 4; ++i) so[w * D + dt * 16 + 4 * fg + i] = oacc[dt][i];
  }
  __syncthreads();
  for (int d = tid; d < D; d += 256) {
    float M = fmaxf(fmaxf(swm[0], swm[1]), fmaxf(swm[2], swm[3]));
    if (own_new) M = fmaxf(M, ssn);
    const float Mu = (M == -INFINITY) ? 0.f : M;
    float o = 0.f, ls = 0.f;
#pragma unroll
    for (int ww = 0; ww < 4; ++ww) {
      const float f = exp2f(swm[ww] - Mu);
      o += so[ww * D + d] * f;
      ls += swl[ww] * f;
    }
    if (own_new) {  // the new token's key: weight exp2(s - M), value straight from the qkv row
      const float f = exp2f(ssn - Mu);
      o += svn[d] * f;
      ls += f;
    }
    dec_store(o, M, ls, b, hk, d, H, nsplit, split, D, po, pm, pl, out, ldo);
  }
  __shared__ int s_last;
  dec_finish<D, 1, XC>(po, pm, pl, H, Hkv, nsplit, b, hk, cnt, out, ldo, &s_last);
}

// ------------------------------------------------------------------------------------------
// Host side: which kernel a launch takes (dec_route; launch_decode shows each route's kernel), then
// one launch site per kernel.
//
// GQA groups (G >= 2) take the MFMA kernel: 1.8x (Llama-3-8B, G=4) to 5x (Llama-3-70B TP=8, G=8)
// over the VALU path (profiles/decode_attn_gqa_mfma_r1.json); the VALU kernel covers the other
// head dim. MHA (G = 1) decode prefetches each wave's next tile (DEC_PFT) when the launch has
// few (row, kv head) pairs (B * Hkv <= 32: latency-bound), else streams with V issued with K; with
// few pairs and splits of at most 512 keys (two tiles per wave) it runs on MFMA instead.
//
// Measured on MI355X (profiles/decode_attn_variants_r1.json): non-temporal K/V loads + V issued with
// K reach 6.5 TB/s for MHA (G = 1, Phi-3); with G >= 2 the extra V registers cost more occupancy
// than they buy, so those keep V after the scores (nt loads only).
//
// xc (same-XCD split exchange; cached ws / counters) and the fused RoPE exist in the MHA kernels
// only; xc needs a few-pairs form, whole groups of 8 pairs, counters and more than one split.
constexpr int kDecPrefetchPairs = 32;
enum DecRoute { DEC_INVALID, DEC_MFMA1, DEC_MHA_STREAM, DEC_MHA_PREFETCH, DEC_MHA_PREFETCH_XC, DEC_GQA_MFMA, DEC_GQA_VALU };

static DecRoute dec_route(int D, int G, int pairs, int chunk, int nsplit, bool has_rope, bool xc, bool has_cnt,
                          bool mfma1_enabled) {
  const bool few = pairs <= kDecPrefetchPairs;
  if (G == 1) {
    if (xc && (!few || pairs % 8 || !has_cnt || nsplit < 2)) return DEC_INVALID;
    if (mfma1_enabled && few && chunk <= 512) return DEC_MFMA1;
    if (xc) return DEC_MHA_PREFETCH_XC;
    return few ? DEC_MHA_PREFETCH : DEC_MHA_STREAM;
  }
  if (xc || has_rope || (G != 2 && G != 4 && G != 8)) return DEC_INVALID;
  return D == 96 ? DEC_GQA_VALU : DEC_GQA_MFMA;
}

struct DecBf16Args : DecArgs {
  const bf16_t* kc; const bf16_t* vc;
  DecRope rope;
};

// Only what dec_route can return at this D is instantiated: a route it cannot return is an error.
template <int D>
static int launch_decode(const DecBf16Args& a, DecRoute route, bool xc) {
#define VALU(GG, VAR) decode_attn_kernel<D, GG, VAR><<<a.grid, 256, 0, a.s>>>(a.q, a.ldq, a.kc, a.vc, DEC_KARGS(a), a.rope)
#define GQA(GG) decode_attn_gqa_kernel<D, GG><<<a.grid, 256, 0, a.s>>>(a.q, a.ldq, a.kc, a.vc, DEC_KARGS(a))
#define M1(XCV, RPV) decode_attn_mfma1_kernel<D, XCV, RPV><<<a.grid, 256, 0, a.s>>>(a.q, a.ldq, a.kc, a.vc, DEC_KARGS(a), a.rope)
  const bool rp = a.rope.cs != nullptr;
  switch (route) {
    case DEC_MFMA1:
      if (xc) { if (rp) M1(true, true); else M1(true, false); }
      else { if (rp) M1(false, true); else M1(false, false); }
      break;
    case DEC_MHA_STREAM: VALU(1, DEC_NT | DEC_VEARLY); break;
    case DEC_MHA_PREFETCH: VALU(1, DEC_NT | DEC_VEARLY | DEC_PFT); break;
    case DEC_MHA_PREFETCH_XC: VALU(1, DEC_NT | DEC_VEARLY | DEC_PFT | DEC_XC); break;
    case DEC_GQA_MFMA:  // D = 64 / 128
      if constexpr (D != 96) { if (a.G == 2) GQA(2); else if (a.G == 4) GQA(4); else GQA(8); }
      else return (int)hipErrorInvalidValue;
      break;
    case DEC_GQA_VALU:  // D = 96
      if constexpr (D == 96) { if (a.G == 2) VALU(2, DEC_NT); else if (a.G == 4) VALU(4, DEC_NT); else VALU(8, DEC_NT); }
      else return (int)hipErrorInvalidValue;
      break;
    default: return (int)hipErrorInvalidValue;
  }
#undef VALU
#undef GQA
#undef M1
  return (int)hipGetLastError();
}

DA_EXPORT int da_malloc_uncached(long long bytes, void** out) {
  hipError_t e = hipExtMallocWithFlags(out, (size_t)bytes, hipDeviceMallocUncached);
  if (e != hipSuccess) return (int)e;
  e = hipMemset(*out, 0, (size_t)bytes);
  if (e != hipSuccess) return (int)e;
  return (int)hipDeviceSynchronize();
}

// The operands: dec_fill (decode_merge.h). xc = 1: same-XCD split exchange (ws / counters in ordinary device memory; the
// caller has checked the launch's workgroup -> XCD round-robin with the placement probe). 0: uncached ws / counters.
DA_EXPORT int da_decode_attn(const void* q, int ldq, const void* k_cache, const void* v_cache, const void* lens,
                             const void* slot, const void* pre, int B, int H, int Hkv, int D, int max_seq, int chunk,
                             int nsplit, float scale, void* ws, void* o, int ldo, void* counters, const void* cos_sin,
                             const void* pos, int xc, void* stream) {
  DecBf16Args a;
  if (dec_fill(a, q, ldq, lens, slot, pre, B, H, Hkv, D, max_seq, chunk, nsplit, scale, ws, o, ldo, counters, cos_sin,
               pos, stream) || !k_cache || !v_cache)
    return (int)hipErrorInvalidValue;
  if (B == 0) return 0;
  a.kc = (const bf16_t*)k_cache; a.vc = (const bf16_t*)v_cache;
  a.rope = DecRope{(bf16_t*)k_cache, (bf16_t*)v_cache, (const float*)cos_sin, (const int*)pos};
  // read once per process; "0" sends the few-pairs MHA launches back to the VALU kernel (bench/decode_mfma1_ab.py)
  static const char* const m1 = getenv("DA_DECODE_MFMA1");
  const DecRoute route = dec_route(D, a.G, B * Hkv, chunk, nsplit, cos_sin != nullptr, xc != 0, counters != nullptr,
                                   !(m1 && m1[0] == '0'));
  const int err = D == 64 ? launch_decode<64>(a, route, xc != 0)
                  : D == 96 ? launch_decode<96>(a, route, xc != 0) : launch_decode<128>(a, route, xc != 0);
  return err ? err : dec_combine(a);
}
