// Batch-1 GEMV on MXFP4 weights (OCP e2m1 codes, one e8m0 power-of-two scale per 32 elements along
// K): the decoder's weight-streaming products at 0.53 bytes per weight, on the structure of the fp8
// GEMV (gemv_w8.hip).
//
//   C[n] = epi( sum_k dq(W4, SE)[n, k] * a'[k] )      a' = the bf16 activation row, optionally
//                                                     RMS-normalised (eps > 0, gamma nullable)
//
//  * a k-block is 1024 elements = 512 B of codes and 32 scale bytes per row, so K % 1024 == 0. Two
//    load forms (LW = code bytes per lane and load):
//      LW = 8   one wave instruction loads one k-block of ONE row (64 lanes x 8 B, coalesced,
//               non-temporal); a lane owns 16 elements, half an MX block;
//      LW = 16  one wave instruction loads two consecutive k-blocks (the two half-waves, 64 x 16 B);
//               a lane owns 32 elements = one whole MX block = one scale byte. A row with an odd
//               number of k-blocks (K = 3072) ends on a half instruction: the upper half-wave's
//               addresses are clamped onto the lower half's block and its scale is replaced by 0,
//               so its products vanish (branch-free);
//  * R rows x U loads per row are issued before any FMA; the scale bytes (one byte load per code
//    load), the activation (LW / 4 16-B loads per lane and round) and the gain vector go through
//    the caches;
//  * v_cvt_scalef32_pk_f32_fp4 (fp4x8_f32, fp4.h) unpacks two codes per instruction and multiplies
//    them by the block's scale (exact), fp32 accumulators per lane, one wave reduction per row; the
//    RMSNorm factor is applied after the reduction, in fp32;
//  * KS = 2: two neighbouring waves of a workgroup split a row's K range and combine their partial
//    sums (and sums of squares) through LDS — long rows on narrow matrices (K = 8192 down projection);
//  * EPI_SWIGLU: a wave owns 2 gate rows and their 2 up rows (16-row interleave) -> 2 outputs.
#include "fp4.h"
#include "gemm.h"

struct GemvW4Args {
  const bf16_t* A; const uint8_t* W; const uint8_t* SE; bf16_t* C;
  const bf16_t* bias; const bf16_t* resid; const bf16_t* gamma;
  int N, K; float eps;
};

template <int LW> struct W4Vec;
template <> struct W4Vec<8> { typedef u32x2_t type; };
template <> struct W4Vec<16> { typedef u32x4_t type; };

template <int EPI, int R, int U, int KS, int LW>
__global__ void __launch_bounds__(256)
gemv_w4_kernel(GemvW4Args p) {
  static_assert(EPI != EPI_SWIGLU || R == 4, "SwiGLU waves own 2 gate + 2 up rows");
  static_assert(KS == 1 || KS == 2, "KS");
  static_assert(LW == 8 || LW == 16, "LW");
  typedef typename W4Vec<LW>::type wvec_t;
  constexpr int EL = LW * 2;   // elements a lane owns per load
  constexpr int EB = EL * 64;  // elements one wave instruction covers in a row: 1024 | 2048
  constexpr int NA = EL / 8;   // 16-B activation loads per lane and load
  const int lane = threadIdx.x & 63;
  const int wv = blockIdx.x * 4 + (threadIdx.x >> 6);  // global wave index
  const int wg = wv / KS, ks = wv % KS;                 // row group, K part
  int rows[R];
  if constexpr (EPI == EPI_SWIGLU) {
    const int g = wg >> 3, t = wg & 7;
#pragma unroll
    for (int r = 0; r < R; ++r) rows[r] = g * 32 + 2 * t + (r & 1) + (r >> 1) * 16;
  } else {
#pragma unroll
    for (int r = 0; r < R; ++r) rows[r] = wg * R + r;
  }
  if (KS == 1 && rows[0] >= p.N) return;  // KS = 2: every wave reaches the LDS exchange below
  // rows past N are clamped (their sums are never stored): the loads stay branch-free
  const uint8_t* wr[R];
  const uint8_t* sr[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int n = min(rows[r], p.N - 1);
    wr[r] = p.W + (size_t)n * (p.K / 2) + lane * LW;
    sr[r] = p.SE + (size_t)n * (p.K / 32) + lane * EL / 32;
  }
  const bf16_t* ar = p.A + lane * EL;
  const bf16_t* gr = p.gamma ? p.gamma + lane * EL : nullptr;
  const bool rms = p.eps > 0.f;  // fused RMSNorm (gamma null = unit gain, folded into the weights)
  const int nkb = (p.K + EB - 1) / EB;
  const int kb0 = ks * nkb / KS, kb1 = (ks + 1) * nkb / KS;
  float acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = 0.f;
  float ss = 0.f;  // sum of squares of the raw input row (this wave's K range)
  for (int kb = kb0; kb < kb1; kb += U) {
    wvec_t wq[U][R];
    unsigned sb[U][R];
    u32x4_t av[U][NA], gv[U][NA];
    bool live[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      int k = min(kb + u, kb1 - 1) * EB;  // tail rounds re-load the last block (cache hit)
      live[u] = true;
      if constexpr (LW == 16) {  // the half instruction that ends a row of an odd number of k-blocks
        live[u] = k + lane * EL < p.K;
        if (!live[u]) k -= 1024;  // the lower half-wave's block: in the row, since K % 1024 == 0
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        wq[u][r] = __builtin_nontemporal_load((const wvec_t*)(wr[r] + k / 2));
        sb[u][r] = sr[r][k / 32];
      }
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        av[u][i] = *(const u32x4_t*)(ar + k + 8 * i);
        if (gr) gv[u][i] = *(const u32x4_t*)(gr + k + 8 * i);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (kb + u >= kb1) break;
      float a[EL];
#pragma unroll
      for (int i = 0; i < NA; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          a[8 * i + 2 * e] = bf2f((bf16_t)(av[u][i][e] & 0xffff));
          a[8 * i + 2 * e + 1] = bf2f((bf16_t)(av[u][i][e] >> 16));
        }
      if (rms) {
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < EL; ++e) s = fmaf(a[e], a[e], s);
        ss += live[u] ? s : 0.f;
      }
      if (gr) {
#pragma unroll
        for (int i = 0; i < NA; ++i)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            a[8 * i + 2 * e] *= bf2f((bf16_t)(gv[u][i][e] & 0xffff));
            a[8 * i + 2 * e + 1] *= bf2f((bf16_t)(gv[u][i][e] >> 16));
          }
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float sc = live[u] ? e8m0_f32(sb[u][r]) : 0.f;  // LW = 8: the lane's half of the MX block
#pragma unroll
        for (int e = 0; e < LW / 4; ++e) {  // word e = weights 8e .. 8e+7 of this lane's EL
          float wf[8];
          fp4x8_f32(wq[u][r][e], sc, wf);
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[r] = fmaf(wf[j], a[8 * e + j], acc[r]);
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = wave_sum(acc[r]);
  if (rms) ss = wave_sum(ss);
  if constexpr (KS == 2) {
    __shared__ float xch[4][R + 1];
    const int w = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < R; ++r) xch[w][r] = acc[r];
      xch[w][R] = ss;
    }
    __syncthreads();
    if (ks != 0 || rows[0] >= p.N) return;
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] += xch[w + 1][r];
    ss += xch[w + 1][R];
  }
  const float inv = rms ? rsqrtf(ss / p.K + p.eps) : 1.f;
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] *= inv;
  if (lane != 0) return;
  if constexpr (EPI == EPI_SWIGLU) {
    const int g = wg >> 3, t = wg & 7;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int o = g * 16 + 2 * t + j;
      if (o < p.N / 2) p.C[o] = f2bf(silu(acc[j]) * acc[2 + j]);
    }
  } else {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int n = rows[r];
      if (n >= p.N) continue;
      float v = acc[r];
      if (p.bias) v += bf2f(p.bias[n]);
      if constexpr (EPI == EPI_RESID) v += bf2f(p.resid[n]);
      p.C[n] = f2bf(v);
    }
  }
}

// EPI_NONE also serves EPI_BIAS (the bias pointer is the switch).
template <int R, int U, int KS, int LW>
static int launch_gemv_w4_r(const GemvW4Args& a, int epi, hipStream_t s) {
  const int waves = (a.N + R - 1) / R * KS;
  dim3 grid((waves + 3) / 4), block(256);
  if (epi == EPI_RESID) gemv_w4_kernel<EPI_RESID, R, U, KS, LW><<<grid, block, 0, s>>>(a);
  else gemv_w4_kernel<EPI_NONE, R, U, KS, LW><<<grid, block, 0, s>>>(a);
  return (int)hipGetLastError();
}

template <int U, int LW>
static int launch_gemv_w4_swiglu(const GemvW4Args& a, hipStream_t s) {
  dim3 grid((a.N / 4 + 3) / 4), block(256);
  gemv_w4_kernel<EPI_SWIGLU, 4, U, 1, LW><<<grid, block, 0, s>>>(a);
  return (int)hipGetLastError();
}

template <int R, int KS, int LW>
static int launch_gemv_w4_u(const GemvW4Args& a, int epi, int u, hipStream_t s) {
  switch (u) {
    case 1: return launch_gemv_w4_r<R, 1, KS, LW>(a, epi, s);
    case 2: return launch_gemv_w4_r<R, 2, KS, LW>(a, epi, s);
    case 3: return launch_gemv_w4_r<R, 3, KS, LW>(a, epi, s);
    default: return launch_gemv_w4_r<R, 4, KS, LW>(a, epi, s);
  }
}

// Loads in flight per row and round: the wave's whole K range when it is at most 4 loads (K = 3072
// at LW = 8: 3 loads, one round, no clamped duplicate), 4 per round otherwise.
static int gemv_w4_u(int nkb_wave) { return nkb_wave < 4 ? nkb_wave : 4; }

// R / U / KS / LW per shape, from the sweep over the five Phi-3-mini batch-1 products on an MI355X
// (bench/w4_sweep.py, profiles/w4/sweep.jsonl; us per launch, weights cold; best arm, then the best
// of the other load form and the nearest losers):
//   9216 x 3072          R4 U3 LW8 6.64   (R2 U3 LW8 6.66, R1 U3 LW8 7.44; best LW16: R2 U2 8.18)
//   32064 x 3072         R4 U3 LW8 13.79  (R4 U1 LW8 14.33, R2 U3 LW8 14.81; best LW16: R4 U2 17.87)
//   3072 x 3072          R1 U3 LW8 3.90   (R2 U3 LW8 4.10, R1 U2 LW8 4.24; best LW16: R1 U2 4.37)
//   3072 x 8192          R2 U1 KS2 LW16 5.71  (R2 U4 KS2 LW8 5.79, R2 U2 KS2 LW8 5.89; best KS1: R1 U2 LW16 6.27)
//   16384 x 3072 SwiGLU  R4 U3 LW8 8.67   (U1 8.81, U2 10.15; best LW16: U2 10.49)
// The 8-B load form wins wherever a row has an odd number of k-blocks (every K = 3072 product: the
// 16-B form spends half an instruction on its clamped tail) and is level on K = 8192 (1.4 %, inside
// the run-to-run spread), so the library carries LW = 8 only. Rows per wave as the fp8 GEMV, with
// four rows per wave from 16384 weight rows (the LM head: 7 % over two rows; level at 9216).
static int launch_gemv_w4(const GemvW4Args& a, int epi, hipStream_t s) {
  const int nkb = a.K / 1024;
  if (epi == EPI_SWIGLU) {
    switch (gemv_w4_u(nkb)) {
      case 1: return launch_gemv_w4_swiglu<1, 8>(a, s);
      case 2: return launch_gemv_w4_swiglu<2, 8>(a, s);
      case 3: return launch_gemv_w4_swiglu<3, 8>(a, s);
      default: return launch_gemv_w4_swiglu<4, 8>(a, s);
    }
  }
  if (a.N >= 16384) return launch_gemv_w4_u<4, 1, 8>(a, epi, gemv_w4_u(nkb), s);
  if (a.N >= 8192) return launch_gemv_w4_u<2, 1, 8>(a, epi, gemv_w4_u(nkb), s);
  // long rows on a narrow matrix (down projection, K = 8192): two waves per row, two rows per pair
  if (nkb >= 8 && nkb % 2 == 0) return launch_gemv_w4_u<2, 2, 8>(a, epi, gemv_w4_u(nkb / 2), s);
  return launch_gemv_w4_u<1, 1, 8>(a, epi, gemv_w4_u(nkb), s);
}

static bool gemv_w4_args_ok(int N, int K, int epi) {
  if (N <= 0 || K <= 0 || K % 1024 || N % 4) return false;
  if (epi == EPI_SWIGLU) return N % 32 == 0;
  return epi == EPI_NONE || epi == EPI_BIAS || epi == EPI_RESID;
}

// C[1, N'] = epi(A[1, K] . dq(W4, SE)[N, K]^T), N' = N / 2 for EPI_SWIGLU. W4: e2m1 codes [N, K/2],
// two per byte (element 2j in bits 3:0 of byte j); SE: e8m0 scale bytes [N, K/32]; A / C / bias /
// resid / gamma bf16. eps > 0 fuses RMSNorm(A) (gamma nullable).
DA_EXPORT int da_gemv_w4(const void* A, const void* W4, const void* SE, void* C, const void* bias, const void* resid,
                         int N, int K, int epi, const void* gamma, float eps, void* stream) {
  if (!gemv_w4_args_ok(N, K, epi) || !A || !W4 || !SE || !C) return (int)hipErrorInvalidValue;
  if (epi == EPI_RESID && !resid) return (int)hipErrorInvalidValue;
  if (gamma && !(eps > 0.f)) return (int)hipErrorInvalidValue;
  GemvW4Args a{(const bf16_t*)A, (const uint8_t*)W4, (const uint8_t*)SE, (bf16_t*)C, (const bf16_t*)bias,
               (const bf16_t*)resid, (const bf16_t*)gamma, N, K, eps};
  return launch_gemv_w4(a, epi, (hipStream_t)stream);
}

#ifdef DA_GEMV_W4_SWEEP
// Sweep build only (bench/w4_sweep.py compiles this file on its own with -DDA_GEMV_W4_SWEEP): every
// R / U / KS / LW arm behind one entry, to pick the dispatch above. Not part of the kernel library.
template <int R, int KS, int LW>
static int sweep_u(const GemvW4Args& a, int epi, int u, hipStream_t s) {
  switch (u) {
    case 1: return launch_gemv_w4_r<R, 1, KS, LW>(a, epi, s);
    case 2: return launch_gemv_w4_r<R, 2, KS, LW>(a, epi, s);
    case 3: return launch_gemv_w4_r<R, 3, KS, LW>(a, epi, s);
    case 4: return launch_gemv_w4_r<R, 4, KS, LW>(a, epi, s);
    default: return (int)hipErrorInvalidValue;
  }
}

template <int LW>
static int sweep_lw(const GemvW4Args& a, int epi, int R, int U, int KS, hipStream_t s) {
  if (epi == EPI_SWIGLU) {
    if (R != 4 || KS != 1) return (int)hipErrorInvalidValue;
    switch (U) {
      case 1: return launch_gemv_w4_swiglu<1, LW>(a, s);
      case 2: return launch_gemv_w4_swiglu<2, LW>(a, s);
      case 3: return launch_gemv_w4_swiglu<3, LW>(a, s);
      case 4: return launch_gemv_w4_swiglu<4, LW>(a, s);
      default: return (int)hipErrorInvalidValue;
    }
  }
  if (KS == 2) {
    switch (R) {
      case 1: return sweep_u<1, 2, LW>(a, epi, U, s);
      case 2: return sweep_u<2, 2, LW>(a, epi, U, s);
      case 4: return sweep_u<4, 2, LW>(a, epi, U, s);
      default: return (int)hipErrorInvalidValue;
    }
  }
  switch (R) {
    case 1: return sweep_u<1, 1, LW>(a, epi, U, s);
    case 2: return sweep_u<2, 1, LW>(a, epi, U, s);
    case 4: return sweep_u<4, 1, LW>(a, epi, U, s);
    default: return (int)hipErrorInvalidValue;
  }
}

DA_EXPORT int da_gemv_w4_sweep(const void* A, const void* W4, const void* SE, void* C, const void* bias,
                               const void* resid, int N, int K, int epi, const void* gamma, float eps, int R, int U,
                               int KS, int LW, void* stream) {
  if (!gemv_w4_args_ok(N, K, epi) || (KS != 1 && KS != 2)) return (int)hipErrorInvalidValue;
  if (KS == 2 && (K + LW * 128 - 1) / (LW * 128) < 2) return (int)hipErrorInvalidValue;
  if (epi == EPI_RESID && !resid) return (int)hipErrorInvalidValue;
  GemvW4Args a{(const bf16_t*)A, (const uint8_t*)W4, (const uint8_t*)SE, (bf16_t*)C, (const bf16_t*)bias,
               (const bf16_t*)resid, (const bf16_t*)gamma, N, K, eps};
  hipStream_t s = (hipStream_t)stream;
  if (LW == 8) return sweep_lw<8>(a, epi, R, U, KS, s);
  if (LW == 16) return sweep_lw<16>(a, epi, R, U, KS, s);
  return (int)hipErrorInvalidValue;
}
#endif
