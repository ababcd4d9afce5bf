// bf16 GEMM on gfx950 MFMA with fused epilogues.
//
//   C[M, N] = epi( A[M, K] · W[N, K]^T )       (nn.Linear layout: both operands K-contiguous)
//
// Design (MI355X-first, see /opt/skills/guides/cdna_hip_programming.md §5):
//  * v_mfma_f32_16x16x32_bf16, 4 waves per workgroup, each wave owns a (BM/WM)x(BN/WN) sub-tile
//    indexed by fragment repeat (acc[FM][FN]), never by wave position.
//  * BK = 64, double-buffered LDS with register-staged prefetch (issue global loads for tile t+1
//    before the MFMAs of tile t, write them to the other LDS buffer after: Guideline 15 / T14).
//  * LDS rows are 128 B; 16-B chunks XOR-swizzled by ((row>>1)&7) so the 16 rows read by one
//    ds_read_b128 lane group land on 16 distinct slots of the 256-B bank row (conflict-free).
//  * bijective XCD remap + grouped-M tile order so neighbouring tiles share an XCD L2 (T1).
//  * epilogue staged through LDS in fp32, then 16-B coalesced stores with bias / GELU / SwiGLU /
//    residual fused (the reference outsources all of this to OpenAI).
//  * split-K writes fp32 partials; gemm_splitk_reduce applies the same epilogue.
#include "fp8.h"
#include "gemm.h"

template <int BM, int BN, int WM, int WN, int EPI, int PF = 1>
__global__ void __launch_bounds__(256)
gemm_bf16_kernel(GemmArgs p) {
  constexpr bool W8 = false, W_NT = false;
#include "gemm_tile_body.inc"
}

// Split-K reduction + epilogue. One thread per 8 output elements (16-B stores).
// ssq_in (nullable): deferred RMSNorm of the product's rows — the A rows were the raw residual
// stream, so by linearity out[m, :] = inv[m] * (A W^T)[m, :], inv[m] = rsqrt(sum_p ssq_in[p][m] /
// norm_k + eps) over the producer's `parts` row sums ([parts][64] floats; gains folded into W).
__global__ void __launch_bounds__(256)
gemm_splitk_reduce(const float* __restrict__ ws, int splits, int M, int N, int epi,
                   const bf16_t* __restrict__ bias, const bf16_t* __restrict__ resid, int ldr,
                   bf16_t* __restrict__ C, int ldc, const float* __restrict__ ssq_in = nullptr, int parts = 0,
                   int norm_k = 1, float eps = 0.f) {
  const int nout = (epi == EPI_SWIGLU) ? N / 2 : N;
  const int chunks = nout / 8;
  const size_t total = (size_t)M * chunks;
  for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < total;
       idx += (size_t)gridDim.x * blockDim.x) {
    const int m = (int)(idx / chunks), oc = (int)(idx % chunks) * 8;
    float inv = 1.f;
    if (ssq_in) {  // a handful of L2-resident floats per row (fixed summation order)
      inv = rsqrtf(sum_strided(ssq_in + m, parts, 64) / norm_k + eps);
    }
    float v[8];
    if (epi == EPI_SWIGLU) {
      const int grp = oc / 16, within = oc % 16;
      const int gc = grp * 32 + within;
      float g[8], u[8];
      sum_rows8(ws + (size_t)m * N + gc, splits, (size_t)M * N, g);
      sum_rows8(ws + (size_t)m * N + gc + 16, splits, (size_t)M * N, u);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = silu(g[e] * inv) * (u[e] * inv);
    } else {
      sum_rows8(ws + (size_t)m * N + oc, splits, (size_t)M * N, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] *= inv;
      if (bias) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += bf2f(bias[oc + e]);
      }
      if (epi == EPI_GELU) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = gelu_erf(v[e]);
      }
      if (epi == EPI_RESID) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += bf2f(resid[(size_t)m * ldr + oc + e]);
      }
    }
    *(u32x4_t*)(C + (size_t)m * ldc + oc) =
        u32x4_t{pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]), pack_bf2(v[4], v[5]), pack_bf2(v[6], v[7])};
  }
}

// ------------------------------------------------------------------------------------------
// GEMV (M = 1: the batch-1 decode step that sets cache-miss latency). Pure weight streaming:
// every wave instruction loads 1 KiB of ONE weight row (64 lanes x 16 B, fully coalesced,
// non-temporal), R rows x U k-blocks of loads are in flight per wave before any FMA, the 8-wide
// dot products accumulate in fp32 per lane and each row is reduced across the wave once.
// The activation row (K bf16) is read through the caches (every wave reads the same vector).
// EPI_SWIGLU: a wave owns 2 gate rows and their 2 up rows (16-row interleave) -> 2 outputs.
// KS = 2: two neighbouring waves of a workgroup split a row's K range (long rows on narrow
// matrices: the K=8192 down projection has 3072 rows, one 16 KiB row per wave was two dependent
// HBM round trips at U=8) and combine their partial sums through LDS.
template <int EPI, int R, int U, int KS = 1>
__global__ void __launch_bounds__(256)
gemv_kernel(GemmArgs p) {
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
  const bf16_t* wr[R];
#pragma unroll
  for (int r = 0; r < R; ++r) wr[r] = p.W + (size_t)min(rows[r], p.N - 1) * p.K + lane * 8;
  const bf16_t* ar = p.A + lane * 8;
  const bf16_t* gr = p.gamma ? p.gamma + lane * 8 : nullptr;
  // fused RMSNorm: eps > 0 (gamma null = unit gain: the decoder folds RMSNorm gains into the
  // following weights at load, so the GEMV streams no gain vector)
  const bool rms = p.eps > 0.f;
  const int nkb = p.K / 512;
  const int kb0 = ks * nkb / KS, kb1 = (ks + 1) * nkb / KS;
  float acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = 0.f;
  float ss = 0.f;  // fused RMSNorm: sum of squares of the raw input row (the wave's K range)
  for (int kb = kb0; kb < kb1; kb += U) {
    u32x4_t wv[U][R], av[U], gv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = min(kb + u, kb1 - 1) * 512;
#pragma unroll
      for (int r = 0; r < R; ++r) wv[u][r] = __builtin_nontemporal_load((const u32x4_t*)(wr[r] + k));
      av[u] = *(const u32x4_t*)(ar + k);
      if (gr) gv[u] = *(const u32x4_t*)(gr + k);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (kb + u >= kb1) break;
      float a[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        a[2 * e] = bf2f((bf16_t)(av[u][e] & 0xffff));
        a[2 * e + 1] = bf2f((bf16_t)(av[u][e] >> 16));
      }
      if (rms) {
#pragma unroll
        for (int e = 0; e < 4; ++e) ss = fmaf(a[2 * e], a[2 * e], fmaf(a[2 * e + 1], a[2 * e + 1], ss));
      }
      if (gr) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          a[2 * e] *= bf2f((bf16_t)(gv[u][e] & 0xffff));
          a[2 * e + 1] *= bf2f((bf16_t)(gv[u][e] >> 16));
        }
      }
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          acc[r] = fmaf(bf2f((bf16_t)(wv[u][r][e] & 0xffff)), a[2 * e], acc[r]);
          acc[r] = fmaf(bf2f((bf16_t)(wv[u][r][e] >> 16)), a[2 * e + 1], acc[r]);
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
  if (rms) {
    const float inv = rsqrtf(ss / p.K + p.eps);
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] *= inv;
  }
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
      if constexpr (EPI == EPI_GELU) v = gelu_erf(v);
      if constexpr (EPI == EPI_RESID) v += bf2f(p.resid[n]);
      p.C[n] = f2bf(v);
    }
  }
}

template <int R, int U, int KS = 1>
static int launch_gemv_r(const GemmArgs& a, int epi, hipStream_t s) {
  const int waves = (a.N + R - 1) / R * KS;
  dim3 grid((waves + 3) / 4), block(256);
  switch (epi) {
    case EPI_NONE: gemv_kernel<EPI_NONE, R, U, KS><<<grid, block, 0, s>>>(a); break;
    case EPI_BIAS: gemv_kernel<EPI_BIAS, R, U, KS><<<grid, block, 0, s>>>(a); break;
    case EPI_GELU: gemv_kernel<EPI_GELU, R, U, KS><<<grid, block, 0, s>>>(a); break;
    case EPI_RESID: gemv_kernel<EPI_RESID, R, U, KS><<<grid, block, 0, s>>>(a); break;
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

// K-blocks (512 elements = 1 KiB per row) in flight per row: the whole row when it is short
// (K = 3072: 6 blocks, one round of loads and no clamped duplicate loads), 8 per round otherwise.
static int gemv_u(int K, int /*R*/) {
  const int nkb = K / 512;
  if (nkb <= 4) return 4;
  if (nkb == 6) return 6;
  // 8, not the whole row at K = 8192: at U = 16 the compiler sinks the loads to their uses
  // (28 VGPRs, one block in flight) and the down projection drops to ~3 TB/s (measured)
  return 8;
}

template <int R>
static int launch_gemv_ru(const GemmArgs& a, int epi, hipStream_t s) {
  switch (gemv_u(a.K, R)) {
    case 6: return launch_gemv_r<R, 6>(a, epi, s);
    case 8: return launch_gemv_r<R, 8>(a, epi, s);
    default: return launch_gemv_r<R, 4>(a, epi, s);
  }
}

// Rows per wave: enough waves (>= ~4 per SIMD) that the loads in flight cover HBM latency on
// narrow matrices, 4 rows per wave (more bytes per wave) on wide ones.
static int launch_gemv(const GemmArgs& a, int epi, hipStream_t s) {
  if (a.M != 1 || a.K % 512 || a.N % 4) return (int)hipErrorInvalidValue;
  if (epi == EPI_SWIGLU) {
    dim3 grid((a.N / 4 + 3) / 4), block(256);
    switch (gemv_u(a.K, 4)) {
      case 6: gemv_kernel<EPI_SWIGLU, 4, 6><<<grid, block, 0, s>>>(a); break;
      case 8: gemv_kernel<EPI_SWIGLU, 4, 8><<<grid, block, 0, s>>>(a); break;
      default: gemv_kernel<EPI_SWIGLU, 4, 4><<<grid, block, 0, s>>>(a); break;
    }
    return (int)hipGetLastError();
  }
  if (a.N >= 16384) return launch_gemv_ru<4>(a, epi, s);
  if (a.N >= 8192) return launch_gemv_ru<2>(a, epi, s);
  // long rows on a narrow matrix (down projection, K = 8192): two waves per row, 8 blocks each
  if (a.K >= 8192 && a.K % 1024 == 0) return launch_gemv_r<1, 8, 2>(a, epi, s);
  return launch_gemv_ru<1>(a, epi, s);
}

template <int BM, int BN, int WM, int WN, int PF = 1>
static int launch_tile(const GemmArgs& a, int epi, int splits, hipStream_t s) {
  const int ntm = (a.M + BM - 1) / BM, ntn = (a.N + BN - 1) / BN;
  dim3 grid(ntm * ntn, 1, splits), block(256);
  switch (splits > 1 ? (int)EPI_PARTIAL : epi) {
    case EPI_NONE: gemm_bf16_kernel<BM, BN, WM, WN, EPI_NONE, PF><<<grid, block, 0, s>>>(a); break;
    case EPI_BIAS: gemm_bf16_kernel<BM, BN, WM, WN, EPI_BIAS, PF><<<grid, block, 0, s>>>(a); break;
    case EPI_GELU: gemm_bf16_kernel<BM, BN, WM, WN, EPI_GELU, PF><<<grid, block, 0, s>>>(a); break;
    case EPI_SWIGLU: gemm_bf16_kernel<BM, BN, WM, WN, EPI_SWIGLU, PF><<<grid, block, 0, s>>>(a); break;
    case EPI_RESID: gemm_bf16_kernel<BM, BN, WM, WN, EPI_RESID, PF><<<grid, block, 0, s>>>(a); break;
    case EPI_PARTIAL: gemm_bf16_kernel<BM, BN, WM, WN, EPI_PARTIAL, PF><<<grid, block, 0, s>>>(a); break;
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

// Decode tiles (64x128 / 32x128): 4 k-tiles in flight per workgroup (register prefetch depth 4;
// 1 / 2 / 8 measured slower, profiles/decode_gemm_prefetch_sweep_r1.jsonl).
template <int BM, int BN>
static int launch_decode_tile(const GemmArgs& a, int epi, int splits, hipStream_t s) {
  return launch_tile<BM, BN, 1, 4, 4>(a, epi, splits, s);
}

// Split-K reduction fused with the residual add AND the next RMSNorm (decode layers, M <= 64):
// one workgroup per row sums the fp32 partials, adds bias + residual, writes the new residual
// stream row C, then normalises that (bf16-rounded) row: H = C * rsqrt(mean(C^2) + eps) * gamma.
// Replaces reduce + rmsnorm (two launches, two passes over the row) with one.
__global__ void __launch_bounds__(256)
splitk_reduce_resid_rmsnorm(const float* __restrict__ ws, int splits, int M, int N, const bf16_t* __restrict__ bias,
                            const bf16_t* __restrict__ resid, int ldr, bf16_t* __restrict__ C, int ldc,
                            const bf16_t* __restrict__ gamma, float eps, bf16_t* __restrict__ H, int ldh) {
  constexpr int MAXC = 4;  // N <= 8 * 256 * 4 = 8192
  __shared__ float red[16];
  const int m = blockIdx.x;
  const int nch = N / 8;
  float v[MAXC][8];
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int c = threadIdx.x + 256 * i;
    if (c >= nch) continue;
    const int oc = c * 8;
    sum_rows8(ws + (size_t)m * N + oc, splits, (size_t)M * N, v[i]);  // 8 splits' loads in flight
    const u32x4_t r = *(const u32x4_t*)(resid + (size_t)m * ldr + oc);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[i][2 * e] += bf2f((bf16_t)(r[e] & 0xffff)) + (bias ? bf2f(bias[oc + 2 * e]) : 0.f);
      v[i][2 * e + 1] += bf2f((bf16_t)(r[e] >> 16)) + (bias ? bf2f(bias[oc + 2 * e + 1]) : 0.f);
    }
    u32x4_t o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      o[e] = pack_bf2(v[i][2 * e], v[i][2 * e + 1]);
      v[i][2 * e] = bf2f((bf16_t)(o[e] & 0xffff));       // normalise what the stream holds (bf16)
      v[i][2 * e + 1] = bf2f((bf16_t)(o[e] >> 16));
      ss += v[i][2 * e] * v[i][2 * e] + v[i][2 * e + 1] * v[i][2 * e + 1];
    }
    *(u32x4_t*)(C + (size_t)m * ldc + oc) = o;
  }
  const float inv = rsqrtf(block_sum(ss, red) / N + eps);
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int c = threadIdx.x + 256 * i;
    if (c >= nch) continue;
    const u32x4_t g = *(const u32x4_t*)(gamma + c * 8);
    u32x4_t o;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      o[e] = pack_bf2(v[i][2 * e] * inv * bf2f((bf16_t)(g[e] & 0xffff)),
                      v[i][2 * e + 1] * inv * bf2f((bf16_t)(g[e] >> 16)));
    *(u32x4_t*)(H + (size_t)m * ldh + c * 8) = o;
  }
}

// The e4m3 weight copy of the *_w8 entry points: codes [N, K] and fp32 row scales [N], both read 16 B
// at a time.
static bool w8_operands_ok(const void* Wq, const void* sw) {
  return Wq && sw && (uintptr_t)Wq % 16 == 0 && (uintptr_t)sw % 16 == 0;
}

// The fp32 partials of a split-K launch on a weight-streaming decode tile: bf16 weights (a.W), or
// with a.sw set the e4m3 codes a.W points at (gemm_tile_w8.hip: tiles 2 and 9, scaled partials).
static int launch_partials(const GemmArgs& a, int tile, int splits, hipStream_t s) {
  if (a.sw) return launch_gemm_tile_w8(a, tile, EPI_PARTIAL, splits, s);
  return tile == 9   ? launch_tile<128, 64, 2, 2, 4>(a, EPI_PARTIAL, splits, s)
         : tile == 2 ? launch_decode_tile<64, 128>(a, EPI_PARTIAL, splits, s)
                     : launch_decode_tile<32, 128>(a, EPI_PARTIAL, splits, s);
}

// da_gemm_resid_rmsnorm / da_gemm_resid_rmsnorm_w8 (sw: the fp8 form, W = the codes)
static int gemm_resid_rmsnorm(const void* A, int lda, const void* W, const float* sw, void* C, int ldc,
                              const void* bias, const void* resid, int ldr, int M, int N, int K, int tile, int splits,
                              void* ws, const void* gamma, float eps, void* Hout, int ldh, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (K % 64 || N % 8 || N > 8192 || lda % 8 || ldc % 8 || ldh % 8 || !ws || !gamma || !resid || !Hout)
    return (int)hipErrorInvalidValue;
  if (splits < 1 || (K / 64) % splits || M > 128 || (M > 64 && tile != 9)) return (int)hipErrorInvalidValue;
  if (M == 0) return 0;
  GemmArgs a{};
  a.A = (const bf16_t*)A; a.W = (const bf16_t*)W; a.C = (bf16_t*)C;
  a.bias = nullptr; a.resid = nullptr; a.ws = (float*)ws; a.sw = sw;
  a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldc = ldc; a.ldr = ldr; a.k_per_split = K / splits;
  // tile 9 (65..128 rows): one 128x64 weight-streaming tile per 64 weight rows
  const int err = launch_partials(a, tile, splits, s);
  if (err) return err;
  splitk_reduce_resid_rmsnorm<<<M, 256, 0, s>>>((const float*)ws, splits, M, N, (const bf16_t*)bias,
                                                (const bf16_t*)resid, ldr, (bf16_t*)C, ldc, (const bf16_t*)gamma, eps,
                                                (bf16_t*)Hout, ldh);
  DA_LAUNCH_CHECK();
}

// C = resid + A.W^T (+ bias) and H = RMSNorm(C) * gamma in two launches (split-K GEMM + fused
// reduce). M <= 128 (decode; above 64 rows tile 9 only), N % 8 == 0, N <= 8192. ws holds splits * M * N floats.
DA_EXPORT int da_gemm_resid_rmsnorm(const void* A, int lda, const void* W, void* C, int ldc, const void* bias,
                                    const void* resid, int ldr, int M, int N, int K, int tile, int splits, void* ws,
                                    const void* gamma, float eps, void* Hout, int ldh, void* stream) {
  return gemm_resid_rmsnorm(A, lda, W, nullptr, C, ldc, bias, resid, ldr, M, N, K, tile, splits, ws, gamma, eps, Hout,
                            ldh, stream);
}

// da_gemm_resid_rmsnorm on W = Wq (e4m3 bytes [N, K]) times sw (fp32 [N]) per row: tile 2 (M <= 64) or
// tile 9, 1 <= M <= 128; Wq and sw 16-B aligned.
DA_EXPORT int da_gemm_resid_rmsnorm_w8(const void* A, int lda, const void* Wq, const void* sw, void* C, int ldc,
                                       const void* bias, const void* resid, int ldr, int M, int N, int K, int tile,
                                       int splits, void* ws, const void* gamma, float eps, void* Hout, int ldh,
                                       void* stream) {
  if (!w8_operands_ok(Wq, sw) || !A || !C || M < 1 || K < 64 || (tile != 2 && tile != 9) || (tile == 2 && M > 64))
    return (int)hipErrorInvalidValue;
  return gemm_resid_rmsnorm(A, lda, Wq, (const float*)sw, C, ldc, bias, resid, ldr, M, N, K, tile, splits, ws, gamma,
                            eps, Hout, ldh, stream);
}

// Split-K reduce of a residual-producing decode GEMM (33..64 rows) in the gemm_dk layer structure:
// C = resid + sum of the partials (+ bias), and per-row sums of squares of the bf16 rows C holds,
// one per 512-column part ([N / 512][64] floats: a consumer reads N / 512 floats per row). One wave
// per (row, 512 columns): no norm here, so no workgroup has to see a whole row — 64 rows x 6
// blocks instead of the 64 row-workgroups of splitk_reduce_resid_rmsnorm, whose 98 KB of partials
// per row was read by one CU.
__global__ void __launch_bounds__(64)
splitk_reduce_resid_ssq(const float* __restrict__ ws, int splits, int M, int N, const bf16_t* __restrict__ bias,
                        const bf16_t* __restrict__ resid, int ldr, bf16_t* __restrict__ C, int ldc,
                        float* __restrict__ ssq_out) {
  const int m = blockIdx.y, lane = threadIdx.x;
  const int oc = blockIdx.x * 512 + lane * 8;
  float v[8];
  sum_rows8(ws + (size_t)m * N + oc, splits, (size_t)M * N, v);
  const u32x4_t r = *(const u32x4_t*)(resid + (size_t)m * ldr + oc);
  u32x4_t o;
  float sq = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float lo = v[2 * e] + bf2f((bf16_t)(r[e] & 0xffff)) + (bias ? bf2f(bias[oc + 2 * e]) : 0.f);
    const float hi = v[2 * e + 1] + bf2f((bf16_t)(r[e] >> 16)) + (bias ? bf2f(bias[oc + 2 * e + 1]) : 0.f);
    o[e] = pack_bf2(lo, hi);
    const float bl = bf2f((bf16_t)(o[e] & 0xffff)), bh = bf2f((bf16_t)(o[e] >> 16));
    sq += bl * bl + bh * bh;  // what the stream now holds (bf16)
  }
  *(u32x4_t*)(C + (size_t)m * ldc + oc) = o;
  sq = wave_sum(sq);
  if (lane == 0) ssq_out[(size_t)blockIdx.x * 64 + m] = sq;
}

// gemm_dk's contract (DkArgs semantics, csrc/gemm_dk.hip) for 33..64 rows on the 64x128 split-K
// tiles: epi NONE / BIAS / SWIGLU with an optional deferred norm of A's rows (ssq_in: the raw
// residual stream as A, the row scale applied in the reduce), or EPI_RESID with optional per-part
// sums of squares out (ssq_out: [N / 512][64]). splits >= 2 whenever a reduce is needed; ws holds
// splits * M * N floats.
static int gemm_dk_splitk(const void* A, int lda, const void* W, const float* sw, void* C, int ldc, const void* bias,
                          const void* resid, int ldr, int M, int N, int K, int epi, const float* ssq_in,
                          int ssq_parts, int norm_k, float eps, float* ssq_out, void* ws, int splits, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (M < 1 || M > 64 || K % 64 || N % 16 || lda % 8 || ldc % 8 || !ws || splits < 2 || (K / 64) % splits)
    return (int)hipErrorInvalidValue;
  if (epi == EPI_SWIGLU && N % 32) return (int)hipErrorInvalidValue;
  if (epi == EPI_RESID && (!resid || ldr % 8 || ssq_in)) return (int)hipErrorInvalidValue;
  if (ssq_out && (epi != EPI_RESID || N % 512)) return (int)hipErrorInvalidValue;
  if (ssq_in && (ssq_parts < 1 || norm_k < 1 || !(eps > 0.f))) return (int)hipErrorInvalidValue;
  if (epi != EPI_NONE && epi != EPI_BIAS && epi != EPI_SWIGLU && epi != EPI_RESID) return (int)hipErrorInvalidValue;
  GemmArgs a{};
  a.A = (const bf16_t*)A; a.W = (const bf16_t*)W; a.C = (bf16_t*)C;
  a.ws = (float*)ws; a.sw = sw;
  a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldc = ldc; a.ldr = ldr; a.k_per_split = K / splits;
  const int err = launch_partials(a, 2, splits, s);
  if (err) return err;
  if (epi == EPI_RESID && ssq_out) {
    splitk_reduce_resid_ssq<<<dim3(N / 512, M), 64, 0, s>>>((const float*)ws, splits, M, N, (const bf16_t*)bias,
                                                            (const bf16_t*)resid, ldr, (bf16_t*)C, ldc, ssq_out);
    DA_LAUNCH_CHECK();
  }
  const int nout = (epi == EPI_SWIGLU) ? N / 2 : N;
  const size_t work = (size_t)M * (nout / 8);
  const int blocks = (int)((work + 255) / 256);
  gemm_splitk_reduce<<<blocks, 256, 0, s>>>((const float*)ws, splits, M, N, epi, (const bf16_t*)bias,
                                             (const bf16_t*)resid, ldr, (bf16_t*)C, ldc, ssq_in, ssq_parts, norm_k,
                                             eps);
  DA_LAUNCH_CHECK();
}

DA_EXPORT int da_gemm_dk_splitk(const void* A, int lda, const void* W, void* C, int ldc, const void* bias,
                                const void* resid, int ldr, int M, int N, int K, int epi, const float* ssq_in,
                                int ssq_parts, int norm_k, float eps, float* ssq_out, void* ws, int splits,
                                void* stream) {
  return gemm_dk_splitk(A, lda, W, nullptr, C, ldc, bias, resid, ldr, M, N, K, epi, ssq_in, ssq_parts, norm_k, eps,
                        ssq_out, ws, splits, stream);
}

// da_gemm_dk_splitk on W = Wq (e4m3 bytes [N, K]) times sw (fp32 [N]) per row; Wq and sw 16-B aligned.
DA_EXPORT int da_gemm_dk_splitk_w8(const void* A, int lda, const void* Wq, const void* sw, void* C, int ldc,
                                   const void* bias, const void* resid, int ldr, int M, int N, int K, int epi,
                                   const float* ssq_in, int ssq_parts, int norm_k, float eps, float* ssq_out, void* ws,
                                   int splits, void* stream) {
  if (!w8_operands_ok(Wq, sw) || !A || !C || K < 64) return (int)hipErrorInvalidValue;
  return gemm_dk_splitk(A, lda, Wq, (const float*)sw, C, ldc, bias, resid, ldr, M, N, K, epi, ssq_in, ssq_parts,
                        norm_k, eps, ssq_out, ws, splits, stream);
}

// Prefill QKV projection with RoPE + KV-cache write fused into the epilogue (gemm8p EPI_ROPE);
// M >= 256 (the phase-split kernel), N == (H + 2 Hkv) * D, D % 8 == 0. kv_out = 0: the k / v
// columns of C are left unwritten (cache only).
DA_EXPORT int da_gemm_rope(const void* A, int lda, const void* W, void* C, int ldc, int M, int N, int K,
                           const void* pos, const void* slot, const void* cos_sin, void* k_cache, void* v_cache,
                           int H, int Hkv, int D, int max_seq, int kv_out, void* stream) {
  if (K % 64 || K < 128 || N % 8 || lda % 8 || ldc % 8 || D % 8 || M < 256) return (int)hipErrorInvalidValue;
  if (N != (H + 2 * Hkv) * D || !pos || !slot || !cos_sin || !k_cache || !v_cache) return (int)hipErrorInvalidValue;
  GemmArgs a{};
  a.A = (const bf16_t*)A; a.W = (const bf16_t*)W; a.C = (bf16_t*)C;
  a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldc = ldc; a.k_per_split = K;
  a.rope = RopeArgs{(const int*)pos, (const int*)slot, (const float*)cos_sin, (bf16_t*)k_cache, (bf16_t*)v_cache,
                    H, Hkv, D, max_seq, kv_out ? 1 : 0};
  // its own measured rule for the RoPE epilogue, not ops/gemm_plan.py's prefill_bm
  const long t256 = (long)((M + 255) / 256) * ((N + 255) / 256);
  return launch_gemm8p(a, EPI_ROPE, (hipStream_t)stream, t256 >= 256 ? 256 : 128);
}

// tile / splits: chosen by ops/gemm_plan.py (the tile ids' legend is there); tile 0 is an error.
DA_EXPORT int da_gemm_bf16(const void* A, int lda, const void* W, void* C, int ldc,
                           const void* bias, const void* resid, int ldr,
                           int M, int N, int K, int epi, int tile, int splits, void* ws,
                           const void* rms_gamma, float rms_eps, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (K % 64 || N % 8 || lda % 8 || ldc % 8) return (int)hipErrorInvalidValue;
  if (epi == EPI_SWIGLU && N % 32) return (int)hipErrorInvalidValue;
  if (splits < 1) splits = 1;
  if ((K / 64) % splits) return (int)hipErrorInvalidValue;
  if (splits > 1 && ws == nullptr) return (int)hipErrorInvalidValue;
  GemmArgs a{};
  a.A = (const bf16_t*)A; a.W = (const bf16_t*)W; a.C = (bf16_t*)C;
  a.bias = (const bf16_t*)bias; a.resid = (const bf16_t*)resid; a.ws = (float*)ws;
  a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldc = ldc; a.ldr = ldr; a.k_per_split = K / splits;
  a.gamma = (const bf16_t*)rms_gamma; a.eps = rms_eps;
  if ((rms_gamma || rms_eps > 0.f) && tile != 6) return (int)hipErrorInvalidValue;  // fused RMSNorm: GEMV only
  if (tile == 4 || tile == 7 || tile == 10) {
    if (splits != 1 || K < 128) return (int)hipErrorInvalidValue;
    return launch_gemm8p(a, epi, s, tile == 10 ? 128 : 256);
  }
  if (tile == 13) {
    if (splits != 1 || K < 128) return (int)hipErrorInvalidValue;
    return launch_gemm4w(a, epi, s);
  }
  if (tile == 6) return launch_gemv(a, epi, s);
  int err;
  switch (tile) {
    case 1: err = launch_tile<128, 128, 2, 2>(a, epi, splits, s); break;
    case 2: err = launch_decode_tile<64, 128>(a, epi, splits, s); break;
    case 3: err = launch_decode_tile<32, 128>(a, epi, splits, s); break;
    case 8: err = launch_tile<128, 128, 2, 2, 4>(a, epi, splits, s); break;   // mid-M weight streaming
    case 9: err = launch_tile<128, 64, 2, 2, 4>(a, epi, splits, s); break;
    default: return (int)hipErrorInvalidValue;
  }
  if (err || splits == 1) return err;
  const int nout = (epi == EPI_SWIGLU) ? N / 2 : N;
  const size_t work = (size_t)M * (nout / 8);
  int blocks = (int)((work + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  gemm_splitk_reduce<<<blocks, 256, 0, s>>>((const float*)ws, splits, M, N, epi, a.bias, a.resid, ldr,
                                             a.C, ldc);
  DA_LAUNCH_CHECK();
}

// da_gemm_bf16's tiles 2 (64x128) and 9 (128x64) on W = Wq (e4m3 bytes [N, K]) times sw (fp32 [N]) per
// row, 1 <= M <= 128: epi NONE / BIAS / SWIGLU / RESID, split-K through gemm_splitk_reduce. Wq and sw
// 16-B aligned.
DA_EXPORT int da_gemm_tile_w8(const void* A, int lda, const void* Wq, const void* sw, void* C, int ldc,
                              const void* bias, const void* resid, int ldr, int M, int N, int K, int epi, int tile,
                              int splits, void* ws, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!w8_operands_ok(Wq, sw) || !A || !C || M < 1 || M > 128 || K < 64 || (tile != 2 && tile != 9))
    return (int)hipErrorInvalidValue;
  if (K % 64 || N % 8 || lda % 8 || ldc % 8) return (int)hipErrorInvalidValue;
  if (epi != EPI_NONE && epi != EPI_BIAS && epi != EPI_SWIGLU && epi != EPI_RESID) return (int)hipErrorInvalidValue;
  if (epi == EPI_SWIGLU && N % 32) return (int)hipErrorInvalidValue;
  if (epi == EPI_RESID && (!resid || ldr % 8)) return (int)hipErrorInvalidValue;
  if (splits < 1) splits = 1;
  if ((K / 64) % splits) return (int)hipErrorInvalidValue;
  if (splits > 1 && ws == nullptr) return (int)hipErrorInvalidValue;
  GemmArgs a{};
  a.A = (const bf16_t*)A; a.W = (const bf16_t*)Wq; a.C = (bf16_t*)C; a.sw = (const float*)sw;
  a.bias = (const bf16_t*)bias; a.resid = epi == EPI_RESID ? (const bf16_t*)resid : nullptr; a.ws = (float*)ws;
  a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldc = ldc; a.ldr = ldr; a.k_per_split = K / splits;
  const int err = launch_gemm_tile_w8(a, tile, epi, splits, s);
  if (err || splits == 1) return err;
  const int nout = (epi == EPI_SWIGLU) ? N / 2 : N;
  const size_t work = (size_t)M * (nout / 8);
  int blocks = (int)((work + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  gemm_splitk_reduce<<<blocks, 256, 0, s>>>((const float*)ws, splits, M, N, epi, a.bias, a.resid, ldr, a.C, ldc);
  DA_LAUNCH_CHECK();
}
