// Batch-1 GEMV on fp8 (OCP e4m3) weights with per-row fp32 scales: the decoder's weight-streaming
// products at half the bytes of the bf16 GEMV (gemm.hip gemv_kernel, whose structure this keeps).
//
//   C[n] = epi( sw[n] * sum_k W8[n, k] * a'[k] )      a' = the bf16 activation row, optionally
//                                                     RMS-normalised (eps > 0, gamma nullable)
//
//  * every wave instruction loads 1 KiB of ONE weight row (64 lanes x 16 B, coalesced,
//    non-temporal): a k-block is 1024 e4m3 elements, so K % 1024 == 0;
//  * R rows x U k-blocks of weight loads are issued before any FMA; the activation (two 16-B
//    loads per lane per k-block) and the gain vector go through the caches;
//  * v_cvt_pk_f32_fp8 (fp8x4_f32, fp8.h) unpacks two weights per instruction, fp32 accumulators
//    per lane, one wave reduction per row; the row scale and the RMSNorm factor are applied after
//    the reduction, in fp32;
//  * KS = 2: two neighbouring waves of a workgroup split a row's K range and combine their partial
//    sums (and sums of squares) through LDS — long rows on narrow matrices (K = 8192 down projection);
//  * EPI_SWIGLU: a wave owns 2 gate rows and their 2 up rows (16-row interleave) -> 2 outputs; the
//    row scales apply before silu.
#include "fp8.h"
#include "gemm.h"

struct GemvW8Args {
  const bf16_t* A; const uint8_t* W; const float* sw; bf16_t* C;
  const bf16_t* bias; const bf16_t* resid; const bf16_t* gamma;
  int N, K; float eps;
};

template <int EPI, int R, int U, int KS>
__global__ void __launch_bounds__(256)
gemv_w8_kernel(GemvW8Args p) {
  static_assert(EPI != EPI_SWIGLU || R == 4, "SwiGLU waves own 2 gate + 2 up rows");
  static_assert(KS == 1 || KS == 2, "KS");
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
  float sc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int n = min(rows[r], p.N - 1);
    wr[r] = p.W + (size_t)n * p.K + lane * 16;
    sc[r] = p.sw[n];
  }
  const bf16_t* ar = p.A + lane * 16;
  const bf16_t* gr = p.gamma ? p.gamma + lane * 16 : nullptr;
  const bool rms = p.eps > 0.f;  // fused RMSNorm (gamma null = unit gain, folded into the weights)
  const int nkb = p.K / 1024;
  const int kb0 = ks * nkb / KS, kb1 = (ks + 1) * nkb / KS;
  float acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = 0.f;
  float ss = 0.f;  // sum of squares of the raw input row (this wave's K range)
  for (int kb = kb0; kb < kb1; kb += U) {
    u32x4_t wq[U][R], av[U][2], gv[U][2];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = min(kb + u, kb1 - 1) * 1024;  // tail rounds re-load the last block (cache hit)
#pragma unroll
      for (int r = 0; r < R; ++r) wq[u][r] = __builtin_nontemporal_load((const u32x4_t*)(wr[r] + k));
      av[u][0] = *(const u32x4_t*)(ar + k);
      av[u][1] = *(const u32x4_t*)(ar + k + 8);
      if (gr) {
        gv[u][0] = *(const u32x4_t*)(gr + k);
        gv[u][1] = *(const u32x4_t*)(gr + k + 8);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (kb + u >= kb1) break;
      float a[16];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          a[8 * h + 2 * e] = bf2f((bf16_t)(av[u][h][e] & 0xffff));
          a[8 * h + 2 * e + 1] = bf2f((bf16_t)(av[u][h][e] >> 16));
        }
      if (rms) {
#pragma unroll
        for (int e = 0; e < 16; ++e) ss = fmaf(a[e], a[e], ss);
      }
      if (gr) {
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            a[8 * h + 2 * e] *= bf2f((bf16_t)(gv[u][h][e] & 0xffff));
            a[8 * h + 2 * e + 1] *= bf2f((bf16_t)(gv[u][h][e] >> 16));
          }
      }
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) {  // word e = weights 4e .. 4e+3 of this lane's 16
          const f32x4_t wf = fp8x4_f32(wq[u][r][e]);
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[r] = fmaf(wf[j], a[4 * e + j], acc[r]);
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
  for (int r = 0; r < R; ++r) acc[r] *= sc[r] * inv;
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
template <int R, int U, int KS>
static int launch_gemv_w8_r(const GemvW8Args& a, int epi, hipStream_t s) {
  const int waves = (a.N + R - 1) / R * KS;
  dim3 grid((waves + 3) / 4), block(256);
  if (epi == EPI_RESID) gemv_w8_kernel<EPI_RESID, R, U, KS><<<grid, block, 0, s>>>(a);
  else gemv_w8_kernel<EPI_NONE, R, U, KS><<<grid, block, 0, s>>>(a);
  return (int)hipGetLastError();
}

template <int U>
static int launch_gemv_w8_swiglu(const GemvW8Args& a, hipStream_t s) {
  dim3 grid((a.N / 4 + 3) / 4), block(256);
  gemv_w8_kernel<EPI_SWIGLU, 4, U, 1><<<grid, block, 0, s>>>(a);
  return (int)hipGetLastError();
}

template <int R, int KS>
static int launch_gemv_w8_u(const GemvW8Args& a, int epi, int u, hipStream_t s) {
  switch (u) {
    case 1: return launch_gemv_w8_r<R, 1, KS>(a, epi, s);
    case 2: return launch_gemv_w8_r<R, 2, KS>(a, epi, s);
    case 3: return launch_gemv_w8_r<R, 3, KS>(a, epi, s);
    default: return launch_gemv_w8_r<R, 4, KS>(a, epi, s);
  }
}

// K-blocks (1 KiB per row) in flight per row and round: the wave's whole K range when it is at
// most 4 blocks (K = 3072: 3 blocks, one round, no clamped duplicate loads), 4 per round otherwise.
static int gemv_w8_u(int nkb_wave) { return nkb_wave < 4 ? nkb_wave : 4; }

// R / U / KS per shape, from the sweep over the five Phi-3-mini batch-1 products on an MI355X
// (bench/w8_sweep.py, profiles/w8/sweep_first_dispatch.jsonl; us per launch, weights cold):
//   9216 x 3072          R2 U3 7.3   (R1 U3 7.9, R4 U3 7.9)
//   32064 x 3072         R2 U3 18.4  (R4 U3 19.1, R1 U3 21.4)
//   3072 x 3072          R1 U3 4.0   (R2 U3 4.3, R4 U3 4.6)
//   3072 x 8192          R2 U4 KS2 6.9  (R1 U4 KS2 7.3, R1 U4 KS1 7.1)
//   16384 x 3072 SwiGLU  R4 U3 11.7  (U1 12.0, U2 12.2)
// A row has half the k-blocks of the bf16 GEMV's, so matrices from 8192 rows take two rows per wave
// (the bf16 kernel: one) to keep as many bytes in flight per wave; four rows per wave lost everywhere.
static int launch_gemv_w8(const GemvW8Args& a, int epi, hipStream_t s) {
  const int nkb = a.K / 1024;
  if (epi == EPI_SWIGLU) {
    switch (gemv_w8_u(nkb)) {
      case 1: return launch_gemv_w8_swiglu<1>(a, s);
      case 2: return launch_gemv_w8_swiglu<2>(a, s);
      case 3: return launch_gemv_w8_swiglu<3>(a, s);
      default: return launch_gemv_w8_swiglu<4>(a, s);
    }
  }
  if (a.N >= 8192) return launch_gemv_w8_u<2, 1>(a, epi, gemv_w8_u(nkb), s);
  // long rows on a narrow matrix (down projection, K = 8192): two waves per row, two rows per pair
  if (nkb >= 8 && nkb % 2 == 0) return launch_gemv_w8_u<2, 2>(a, epi, gemv_w8_u(nkb / 2), s);
  return launch_gemv_w8_u<1, 1>(a, epi, gemv_w8_u(nkb), s);
}

static bool gemv_w8_args_ok(int N, int K, int epi) {
  if (N <= 0 || K <= 0 || K % 1024 || N % 4) return false;
  if (epi == EPI_SWIGLU) return N % 32 == 0;
  return epi == EPI_NONE || epi == EPI_BIAS || epi == EPI_RESID;
}

// C[1, N'] = epi(sw * (A[1, K] . W8[N, K]^T)), N' = N / 2 for EPI_SWIGLU. W8: e4m3 bytes, row-major;
// sw: fp32 [N]; A / C / bias / resid / gamma bf16. eps > 0 fuses RMSNorm(A) (gamma nullable).
DA_EXPORT int da_gemv_w8(const void* A, const void* W8, const void* sw, void* C, const void* bias, const void* resid,
                         int N, int K, int epi, const void* gamma, float eps, void* stream) {
  if (!gemv_w8_args_ok(N, K, epi) || !A || !W8 || !sw || !C) return (int)hipErrorInvalidValue;
  if (epi == EPI_RESID && !resid) return (int)hipErrorInvalidValue;
  if (gamma && !(eps > 0.f)) return (int)hipErrorInvalidValue;
  GemvW8Args a{(const bf16_t*)A, (const uint8_t*)W8, (const float*)sw, (bf16_t*)C, (const bf16_t*)bias,
               (const bf16_t*)resid, (const bf16_t*)gamma, N, K, eps};
  return launch_gemv_w8(a, epi, (hipStream_t)stream);
}

#ifdef DA_GEMV_W8_SWEEP
// Sweep build only (bench/w8_sweep.py compiles this file on its own with -DDA_GEMV_W8_SWEEP): every
// R / U / KS arm behind one entry, to pick the dispatch above. Not part of the kernel library.
template <int R, int KS>
static int sweep_u(const GemvW8Args& a, int epi, int u, hipStream_t s) {
  switch (u) {
    case 1: return launch_gemv_w8_r<R, 1, KS>(a, epi, s);
    case 2: return launch_gemv_w8_r<R, 2, KS>(a, epi, s);
    case 3: return launch_gemv_w8_r<R, 3, KS>(a, epi, s);
    case 4: return launch_gemv_w8_r<R, 4, KS>(a, epi, s);
    case 8: return launch_gemv_w8_r<R, 8, KS>(a, epi, s);
    default: return (int)hipErrorInvalidValue;
  }
}

DA_EXPORT int da_gemv_w8_sweep(const void* A, const void* W8, const void* sw, void* C, const void* bias,
                               const void* resid, int N, int K, int epi, const void* gamma, float eps, int R, int U,
                               int KS, void* stream) {
  if (!gemv_w8_args_ok(N, K, epi) || (KS == 2 && (K / 1024) % 2)) return (int)hipErrorInvalidValue;
  if (epi == EPI_RESID && !resid) return (int)hipErrorInvalidValue;
  GemvW8Args a{(const bf16_t*)A, (const uint8_t*)W8, (const float*)sw, (bf16_t*)C, (const bf16_t*)bias,
               (const bf16_t*)resid, (const bf16_t*)gamma, N, K, eps};
  hipStream_t s = (hipStream_t)stream;
  if (epi == EPI_SWIGLU) {
    if (R != 4 || KS != 1) return (int)hipErrorInvalidValue;
    switch (U) {
      case 1: return launch_gemv_w8_swiglu<1>(a, s);
      case 2: return launch_gemv_w8_swiglu<2>(a, s);
      case 3: return launch_gemv_w8_swiglu<3>(a, s);
      case 4: return launch_gemv_w8_swiglu<4>(a, s);
      default: return (int)hipErrorInvalidValue;
    }
  }
  if (KS == 2) {
    switch (R) {
      case 1: return sweep_u<1, 2>(a, epi, U, s);
      case 2: return sweep_u<2, 2>(a, epi, U, s);
      case 4: return sweep_u<4, 2>(a, epi, U, s);
      default: return (int)hipErrorInvalidValue;
    }
  }
  switch (R) {
    case 1: return sweep_u<1, 1>(a, epi, U, s);
    case 2: return sweep_u<2, 1>(a, epi, U, s);
    case 4: return sweep_u<4, 1>(a, epi, U, s);
    case 8: return sweep_u<8, 1>(a, epi, U, s);
    default: return (int)hipErrorInvalidValue;
  }
}
#endif
