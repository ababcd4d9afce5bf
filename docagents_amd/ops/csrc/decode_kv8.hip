// fp8 (OCP e4m3) KV cache: the write side (RoPE + per-row quantisation), split-KV decode attention
// over the codes, and the dequantisation of a slot's head for the flash prefill's shared prefix.
//
// Storage: every K row and every V row of one (token, kv head) — D values — is stored as D e4m3
// codes plus ONE fp32 power-of-two scale: the smallest 2^e with amax / 2^e <= 448 (1 for an
// all-zero row): fp8_pow2_scale (fp8.h). code * 2^e is exact in bf16.
//   codes  [slots, Hkv, max_seq, D]  one byte each
//   scales [slots, Hkv, max_seq]     fp32
// A decode-attention launch streams (D + 4) bytes per cached row instead of 2 D.
#include "decode_merge.h"
#include "fp8.h"

// ------------------------------------------------------------------------------------------
// RoPE (in place on the q and k heads of qkv, the roundings of rope_cache_kernel) + quantisation of
// the rotated k row and the v row of every (token, kv head) into the cache at [slot[t], :, pos[t]].
// One half-wave (32 lanes, 4 elements = 2 rotary pairs per lane, D <= 128) per head row: the q heads
// (rotated only), the k heads (rotated, then quantised), the v heads (quantised). amax over the row
// with lane shuffles that stay inside the half-wave.
__global__ void __launch_bounds__(256)
rope_cache_kv8_kernel(bf16_t* __restrict__ qkv, const int* __restrict__ pos, const int* __restrict__ slot,
                      const float* __restrict__ cs, uint8_t* __restrict__ kq, uint8_t* __restrict__ vq,
                      float* __restrict__ ksc, float* __restrict__ vsc, int H, int Hkv, int D, int max_seq,
                      int rotate_q) {
  const int t = blockIdx.x;
  const int item = (blockIdx.y * 256 + threadIdx.x) >> 5;
  const int l = threadIdx.x & 31;
  const int Hq = rotate_q ? H : 0;
  const int nitems = Hq + 2 * Hkv;
  const bool live = item < nitems;
  const int j = live ? item : nitems - 1;  // dead half-waves still take part in the shuffles
  const int head = j < Hq ? j : H + (j - Hq);  // head row within [q | k | v]
  const bool rot = j < Hq + Hkv, quant = j >= Hq;
  const bool act = live && l < D / 4;
  const int p = pos[t], s = slot[t];
  DA_ASSERT(p >= 0 && p < max_seq && s >= 0);
  bf16_t* hp = qkv + (size_t)t * (H + 2 * Hkv) * D + (size_t)head * D + l * 4;
  u32x2_t a = {0u, 0u};
  if (act) a = *(const u32x2_t*)hp;
  if (rot && act) {
    const f32x4_t c = *(const f32x4_t*)(cs + ((size_t)p * (D / 2) + l * 2) * 2);  // (cos, sin) of 2 pairs
    const float cc[2] = {c[0], c[2]}, sn[2] = {c[1], c[3]};
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const float x1 = bf2f(a[e] & 0xffff), x2 = bf2f(a[e] >> 16);
      const float o1 = x1 * cc[e] - x2 * sn[e];
      const float o2 = x2 * cc[e] + x1 * sn[e];
      a[e] = pack_bf2(o1, o2);
    }
    *(u32x2_t*)hp = a;
  }
  const float x[4] = {bf2f(a[0] & 0xffff), bf2f(a[0] >> 16), bf2f(a[1] & 0xffff), bf2f(a[1] >> 16)};
  float amax = fmaxf(fmaxf(fabsf(x[0]), fabsf(x[1])), fmaxf(fabsf(x[2]), fabsf(x[3])));
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
  if (!(quant && act)) return;
  float sc, inv;
  fp8_pow2_scale(amax, sc, inv);
  const int hk = (j - Hq) % Hkv;
  const bool isk = j < Hq + Hkv;
  const size_t row = ((size_t)s * Hkv + hk) * max_seq + p;
  *(unsigned*)((isk ? kq : vq) + row * D + l * 4) = f32x4_fp8(x[0], x[1], x[2], x[3], inv);
  if (l == 0) (isk ? ksc : vsc)[row] = sc;
}

DA_EXPORT int da_rope_cache_kv8(void* qkv, const void* pos, const void* slot, const void* cos_sin, void* k_codes,
                                void* v_codes, void* k_scale, void* v_scale, int T, int H, int Hkv, int D, int max_seq,
                                int rotate_q, void* stream) {
  if (D % 8 || D > 128 || D < 8 || H < 1 || Hkv < 1) return (int)hipErrorInvalidValue;
  if (!qkv || !pos || !slot || !cos_sin || !k_codes || !v_codes || !k_scale || !v_scale) return (int)hipErrorInvalidValue;
  if (T == 0) return 0;
  const int items = (rotate_q ? H : 0) + 2 * Hkv;  // half-waves per token, 8 per workgroup
  const dim3 grid(T, (items + 7) / 8);
  rope_cache_kv8_kernel<<<grid, 256, 0, (hipStream_t)stream>>>((bf16_t*)qkv, (const int*)pos, (const int*)slot,
                                                             (const float*)cos_sin, (uint8_t*)k_codes,
                                                             (uint8_t*)v_codes, (float*)k_scale, (float*)v_scale, H,
                                                             Hkv, D, max_seq, rotate_q);
  DA_LAUNCH_CHECK();
}

// ------------------------------------------------------------------------------------------
// The first P keys of one slot, dequantised to bf16 [Hkv, P, D] (exact): the flash prefill's shared
// prefix. One thread per 16 codes.
__global__ void __launch_bounds__(256)
kv8_dequant_kernel(const uint8_t* __restrict__ codes, const float* __restrict__ scale, int slot, int Hkv, int P,
                   int D, int max_seq, bf16_t* __restrict__ out) {
  const int cpr = D / 16;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)Hkv * P * cpr) return;
  const int c = (int)(i % cpr), p = (int)((i / cpr) % P), hk = (int)(i / ((long long)cpr * P));
  const size_t row = ((size_t)slot * Hkv + hk) * max_seq + p;
  const u32x4_t w = *(const u32x4_t*)(codes + row * D + c * 16);
  const float s = scale[row];
  unsigned b[8];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const f32x4_t f = fp8x4_f32(w[e]);
    b[2 * e] = pack_bf2(f[0] * s, f[1] * s);
    b[2 * e + 1] = pack_bf2(f[2] * s, f[3] * s);
  }
  bf16_t* dst = out + ((size_t)hk * P + p) * D + c * 16;
  *(u32x4_t*)dst = u32x4_t{b[0], b[1], b[2], b[3]};
  *(u32x4_t*)(dst + 8) = u32x4_t{b[4], b[5], b[6], b[7]};
}

DA_EXPORT int da_kv8_dequant(const void* codes, const void* scale, int slot, int slots, int Hkv, int P, int D,
                             int max_seq, void* out, void* stream) {
  if (D % 16 || D < 16 || Hkv < 1 || P < 0 || P > max_seq || slot < 0 || slot >= slots || !codes || !scale || !out)
    return (int)hipErrorInvalidValue;
  if (P == 0) return 0;
  const long long n = (long long)Hkv * P * (D / 16);
  kv8_dequant_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(
      (const uint8_t*)codes, (const float*)scale, slot, Hkv, P, D, max_seq, (bf16_t*)out);
  DA_LAUNCH_CHECK();
}

// ------------------------------------------------------------------------------------------
// Split-KV decode attention over the fp8 cache: the structure of decode_attn_kernel<D, G, 3>
// (decode_attn.hip; the streaming form the batch-128 step runs) at half the bytes per key.
//   grid (nsplit, Hkv, B), 4 waves; each wave streams its own 64-key tiles with its own online
//   softmax (no block barrier in the loop); the waves merge once at the end, the splits through
//   dec_store / dec_finish (or decode_combine_kernel).
// A 64-key tile of one kv head is a contiguous [64 x D] block of codes = 64 * D / 16 16-B chunks,
// read as D / 16 fully coalesced non-temporal wave-instructions, V requested together with K, plus
// one 4-B scale per key for K and for V (lane = key). Chunk c of a tile holds key c / (D/16), dims
// 16 * (c % (D/16)) .. +15; v_cvt_pk_f32_fp8 unpacks two codes per instruction in registers. The
// key's scale multiplies its score (after the dot product over the codes), the value's scale its
// probability before P*V, so the payload itself is never rescaled. Accumulation is fp32, on
// two-wide vectors (v_pk_fma_f32).
template <int D, int G>
__global__ void __launch_bounds__(256)
decode_attn_kv8_kernel(const bf16_t* __restrict__ q, int ldq, const uint8_t* __restrict__ kc,
                       const uint8_t* __restrict__ vc, const float* __restrict__ ksc,
                       const float* __restrict__ vsc, const int* __restrict__ lens, const int* __restrict__ slot,
                       const int* __restrict__ pre, int H, int Hkv, int max_seq, int chunk_max, int nsplit,
                       float scale_log2e, float* __restrict__ po, float* __restrict__ pm, float* __restrict__ pl,
                       bf16_t* __restrict__ out, int ldo, int* __restrict__ cnt) {
  constexpr int KT = 64;
  constexpr int CPR = D / 16;                      // 16-B chunks per key row
  constexpr int GCD = (CPR % 8 == 0) ? 8 : ((CPR % 4 == 0) ? 4 : 2);
  constexpr int NSET = CPR / GCD;                  // distinct dim-slots per lane
  constexpr bool SHFL = (64 % CPR) == 0;           // a key's chunks live in one wave-instruction
  constexpr int NWV = 4, NTH = 64 * NWV;
  static_assert(D % 16 == 0 && D <= 128 && NTH >= D, "head dim");
  __shared__ float sq[G][D];
  __shared__ float sp[NWV][G][KT];
  __shared__ float spart[SHFL ? 1 : NWV][SHFL ? 1 : G * KT * CPR];
  __shared__ float so[G == 1 ? 1 : NWV][G][D];
  __shared__ float sacc[G == 1 ? 2 * NSET * 64 * 16 : 1];  // two waves' accumulators at a time
  __shared__ float swm[NWV][G], swl[NWV][G];

  const int split = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
  const int L = lens[b];
  DA_ASSERT(L >= 0 && L <= max_seq && slot[b] >= 0);
  const int chunk = dec_chunk(L, nsplit, chunk_max);
  const int kstart = split * chunk;
  const int kend = min(L, kstart + chunk);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const size_t crow = ((size_t)slot[b] * Hkv + hk) * (size_t)max_seq;  // first cache row of (slot, kv head)
  const int P = pre ? pre[2 * b] : 0;  // shared-prefix keys [0, P) live in slot pre[2b + 1]
  const size_t prow = P ? ((size_t)pre[2 * b + 1] * Hkv + hk) * (size_t)max_seq : crow;
  DA_ASSERT(P >= 0 && P <= L);

  auto ld16 = [&](const uint8_t* p) -> u32x4_t { return __builtin_nontemporal_load((const u32x4_t*)p); };
  // branch-free per lane: chunks / keys past the tile's end read nothing and are zero (code 0 = 0.0)
  auto load_tile = [&](u32x4_t (&kv)[CPR], u32x4_t (&vv)[CPR], float& ks, float& vs, int t0) {
    const int nk = min(KT, kend - t0);
    const int last = nk * CPR - 1;
    const size_t r0 = (t0 < P ? prow : crow) + (size_t)t0;
    const uint8_t* kb = kc + r0 * D;
    const uint8_t* vb = vc + r0 * D;
    if (t0 < P && P < t0 + KT) {
      // the tile that holds key P when P is no multiple of 64: its keys from P on come from the row's
      // own slot (a wave-uniform branch: whole-tile prefixes run the loads below, as they always did)
      const size_t o0 = crow + (size_t)t0;
      const int npre = P - t0, cut = npre * CPR;
#pragma unroll
      for (int i = 0; i < CPR; ++i) {
        const int c = i * 64 + lane;
        kv[i] = (c <= last) ? ld16(kc + (c < cut ? r0 : o0) * D + c * 16) : u32x4_t{0, 0, 0, 0};
        vv[i] = (c <= last) ? ld16(vc + (c < cut ? r0 : o0) * D + c * 16) : u32x4_t{0, 0, 0, 0};
      }
      const size_t rs = (lane < npre ? r0 : o0) + lane;
      ks = lane < nk ? __builtin_nontemporal_load(ksc + rs) : 0.f;
      vs = lane < nk ? __builtin_nontemporal_load(vsc + rs) : 0.f;
      return;
    }
#pragma unroll
    for (int i = 0; i < CPR; ++i) {
      const int c = i * 64 + lane;
      kv[i] = (c <= last) ? ld16(kb + c * 16) : u32x4_t{0, 0, 0, 0};
    }
    ks = lane < nk ? __builtin_nontemporal_load(ksc + r0 + lane) : 0.f;
#pragma unroll
    for (int i = 0; i < CPR; ++i) {
      const int c = i * 64 + lane;
      vv[i] = (c <= last) ? ld16(vb + c * 16) : u32x4_t{0, 0, 0, 0};
    }
    vs = lane < nk ? __builtin_nontemporal_load(vsc + r0 + lane) : 0.f;
  };

  for (int i = tid; i < G * D; i += NTH) {
    const int g = i / D, d = i % D;
    sq[g][d] = bf2f(q[(size_t)b * ldq + (hk * G + g) * D + d]) * scale_log2e;
  }
  if constexpr (G > 1) {
    for (int i = tid; i < NWV * G * D; i += NTH) (&so[0][0][0])[i] = 0.f;
  }
  __syncthreads();

  float m[G], l[G];
  f32x2_t acc[G][NSET][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    m[g] = -INFINITY; l[g] = 0.f;
#pragma unroll
    for (int s = 0; s < NSET; ++s)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[g][s][e] = f32x2_t{0.f, 0.f};
  }

  for (int t0 = kstart + w * KT; t0 < kend; t0 += NWV * KT) {
    u32x4_t kv[CPR], vv[CPR];
    float ks, vs;
    load_tile(kv, vv, ks, vs, t0);
    const int nk = min(KT, kend - t0);
    // ---- scores over the codes ----
#pragma unroll
    for (int i = 0; i < CPR; ++i) {
      const int c = i * 64 + lane;
      const int dp = c % CPR;
      f32x2_t kf[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const f32x4_t f = fp8x4_f32(kv[i][e]);
        kf[2 * e] = f.lo;
        kf[2 * e + 1] = f.hi;
      }
#pragma unroll
      for (int g = 0; g < G; ++g) {
        f32x2_t a2 = {0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const f32x4_t q4 = *(const f32x4_t*)&sq[g][dp * 16 + 4 * e];
          a2 += kf[2 * e] * f32x2_t{q4[0], q4[1]};
          a2 += kf[2 * e + 1] * f32x2_t{q4[2], q4[3]};
        }
        float part = a2[0] + a2[1];
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
    // ---- online softmax; lane = key: the key's scale on its score, the value's on its probability ----
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
      sc = (lane < nk) ? sc * ks : -INFINITY;
      const float tmax = wave_max(sc);
      const float m_new = fmaxf(m[g], tmax);
      const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
      const float alpha = exp2f(m[g] - m_use);
      const float p = exp2f(sc - m_use);
      l[g] = l[g] * alpha + wave_sum(p);
      m[g] = m_new;
      sp[w][g][lane] = p * vs;
#pragma unroll
      for (int st = 0; st < NSET; ++st)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[g][st][e] *= alpha;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // ---- P * V ----
#pragma unroll
    for (int i = 0; i < CPR; ++i) {
      const int c = i * 64 + lane;
      const int key = c / CPR;
      f32x2_t vf[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const f32x4_t f = fp8x4_f32(vv[i][e]);
        vf[2 * e] = f.lo;
        vf[2 * e + 1] = f.hi;
      }
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float pk = sp[w][g][key];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[g][i % NSET][e] += vf[e] * pk;
      }
    }
    __builtin_amdgcn_wave_barrier();
  }

  // ---- merge lanes -> per-wave O, then waves -> block partial ----
  if (lane == 0) {
#pragma unroll
    for (int g = 0; g < G; ++g) { swm[w][g] = m[g]; swl[w][g] = l[g]; }
  }
  if constexpr (G > 1) {
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int st = 0; st < NSET; ++st) {
        const int dp = (lane + 64 * st) % CPR;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          atomicAdd(&so[w][g][dp * 16 + 2 * e], acc[g][st][e][0]);
          atomicAdd(&so[w][g][dp * 16 + 2 * e + 1], acc[g][st][e][1]);
        }
      }
  }
  __syncthreads();
  if constexpr (G == 1) {
    // MHA: every lane parks its accumulators in LDS with plain 16-B stores (two waves per pass, so
    // the buffer stays small enough for 4+ workgroups per CU) and thread d sums the (dim-slot, lane)
    // entries that hold dim d: lane l's slot st holds dims 16 * ((64 st + l) % CPR) .. +15
    const int d = tid, dp = (d >> 4) % CPR, e = d & 15;
    const float M = fmaxf(fmaxf(swm[0][0], swm[1][0]), fmaxf(swm[2][0], swm[3][0]));
    const float Mu = (M == -INFINITY) ? 0.f : M;
    float o = 0.f, ls = 0.f;
#pragma unroll
    for (int pass = 0; pass < NWV / 2; ++pass) {
      if ((w >> 1) == pass) {
#pragma unroll
        for (int st = 0; st < NSET; ++st) {
          float* dst = &sacc[(((w & 1) * NSET + st) * 64 + lane) * 16];
#pragma unroll
          for (int k4 = 0; k4 < 4; ++k4)
            *(f32x4_t*)(dst + 4 * k4) = f32x4_t{acc[0][st][2 * k4][0], acc[0][st][2 * k4][1],
                                                acc[0][st][2 * k4 + 1][0], acc[0][st][2 * k4 + 1][1]};
        }
      }
      __syncthreads();
      if (d < D) {
#pragma unroll
        for (int w2 = 0; w2 < 2; ++w2) {
          const int ww = 2 * pass + w2;
          float ow = 0.f;
#pragma unroll
          for (int st = 0; st < NSET; ++st) {
            const int l0 = ((dp - 64 * st) % CPR + CPR) % CPR;
#pragma unroll
            for (int j = 0; j < (64 + CPR - 1) / CPR; ++j) {
              const int ln = l0 + j * CPR;
              if (ln < 64) ow += sacc[((w2 * NSET + st) * 64 + ln) * 16 + e];
            }
          }
          const float f = exp2f(swm[ww][0] - Mu);
          o += ow * f;
          ls += swl[ww][0] * f;
        }
      }
      __syncthreads();
    }
    if (d < D) dec_store(o, M, ls, b, hk, d, H, nsplit, split, D, po, pm, pl, out, ldo);
  } else {
    for (int i = tid; i < G * D; i += NTH) {
      const int g = i / D, d = i % D;
      const float M = fmaxf(fmaxf(swm[0][g], swm[1][g]), fmaxf(swm[2][g], swm[3][g]));
      const float Mu = (M == -INFINITY) ? 0.f : M;
      float o = 0.f, ls = 0.f;
#pragma unroll
      for (int ww = 0; ww < NWV; ++ww) {
        const float f = exp2f(swm[ww][g] - Mu);
        o += so[ww][g][d] * f;
        ls += swl[ww][g] * f;
      }
      dec_store(o, M, ls, b, hk * G + g, d, H, nsplit, split, D, po, pm, pl, out, ldo);
    }
  }
  __shared__ int s_last;
  dec_finish<D, G>(po, pm, pl, H, Hkv, nsplit, b, hk, cnt, out, ldo, &s_last);
}

struct DecKv8Args : DecArgs {
  const uint8_t* kc; const uint8_t* vc;  // codes
  const float* ksc; const float* vsc;    // row scales
};

template <int D>
static int launch_decode_kv8(const DecKv8Args& a) {
#define DEC8(GG) decode_attn_kv8_kernel<D, GG><<<a.grid, 256, 0, a.s>>>(a.q, a.ldq, a.kc, a.vc, a.ksc, a.vsc, DEC_KARGS(a))
  switch (a.G) {
    case 1: DEC8(1); break;
    case 2: DEC8(2); break;
    case 4: DEC8(4); break;
    case 8: DEC8(8); break;
    default: return (int)hipErrorInvalidValue;
  }
#undef DEC8
  return (int)hipGetLastError();
}

// As da_decode_attn without the fused RoPE and the same-XCD exchange: ws holds B*H*nsplit*(D+2)
// floats; counters (nullable) int32 [B * Hkv], zero, left zero — with them, ws and counters are
// uncached allocations and the last split merges in the kernel; without, a combine launch follows.
DA_EXPORT int da_decode_attn_kv8(const void* q, int ldq, const void* k_codes, const void* v_codes,
                                 const void* k_scale, const void* v_scale, const void* lens, const void* slot,
                                 const void* pre, int B, int H, int Hkv, int D, int max_seq, int chunk, int nsplit,
                                 float scale, void* ws, void* o, int ldo, void* counters, void* stream) {
  DecKv8Args a;
  if (dec_fill(a, q, ldq, lens, slot, pre, B, H, Hkv, D, max_seq, chunk, nsplit, scale, ws, o, ldo, counters, nullptr,
               nullptr, stream) || !k_codes || !v_codes || !k_scale || !v_scale)
    return (int)hipErrorInvalidValue;
  if (B == 0) return 0;
  a.kc = (const uint8_t*)k_codes; a.vc = (const uint8_t*)v_codes;
  a.ksc = (const float*)k_scale; a.vsc = (const float*)v_scale;
  const int err = D == 64 ? launch_decode_kv8<64>(a) : D == 96 ? launch_decode_kv8<96>(a) : launch_decode_kv8<128>(a);
  return err ? err : dec_combine(a);
}
