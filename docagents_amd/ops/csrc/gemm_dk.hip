// Decode GEMM for 2 <= M <= 64 rows with NO split-K partials (gemm_dk).
//
//   C[M, N'] = epi( rownorm(A)[M, K] . W[N, K]^T )
//
// Why: the 64x128 / 32x128 weight-streaming tiles (gemm.hip) need split-K to put enough workgroups
// on 256 CUs, and every split-K GEMM is followed by a reduce launch. In a 32-layer Phi-3 chain at
// M = 16 / 64 those reduces are 4 launches x ~4.7 us per layer — 26 % of the chain
// (rocprofv3 --kernel-trace of bench/midm_chain.py, profiles/r3/chainprof/). Here the K split lives
// INSIDE the workgroup: 4 waves each stream a quarter of K for the same BN weight rows and the four
// accumulator sets are summed through LDS at the end, so a workgroup owns finished outputs and the
// epilogue (bias / residual / SwiGLU) runs in the same launch. Narrow tiles (BN = 16..64 rows of W)
// give >= 192 workgroups without any global split.
//
// Operands go straight from global memory to the MFMA registers (v_mfma_f32_16x16x32_bf16: lane l
// holds row 16 i + (l & 15), k chunk 8 (l >> 4)); nothing is shared between the waves of a workgroup
// (disjoint K quarters), so there is no LDS staging and no barrier in the main loop. PF k-steps of
// A and W fragments are in flight per wave (counted vmcnt waits: the ring is indexed by unrolled
// slot, loads issued in k order).
//
// Deferred RMSNorm (NORM): the decode layer's norms ride here instead of in a reduce launch. The
// producer of the residual stream (EPI_RESID) writes, next to x, per-(workgroup, row) sums of squares
// of its bf16 output slice (ssq_out [parts][64]); the consumer reads x itself as A and scales each A
// fragment by inv[m] = rsqrt(sum_parts / norm_k + eps) before the MFMA (bf16-rounded exactly like
// the rmsnorm kernel's output; the RMSNorm gains are folded into W at load, models/llama.py).
//
// The kernel body is gemm_dk_body.inc, shared with gemm_dk_w8.hip; here it runs on the bf16 weight
// source (DkWBf16, gemm_dk.h), which also has the two row blocks for 33..64 rows.
#include "gemm_dk.h"

template <int BM, int BN, int EPI, bool NORM, int PF>
__global__ void __launch_bounds__(256)
gemm_dk_kernel(DkArgs p) {
  using WS = DkWBf16;
#include "gemm_dk_body.inc"
}

// Chunks in flight per workgroup: ~64 KB of W (128 / BN chunks of BN x 512 B) within ~160 VGPRs of
// register staging.
static constexpr int dk_pf(int BM, int BN) {
  int pf = 128 / BN;
  while (pf > 1 && pf * (BN + BM) / 2 > 160) pf /= 2;
  return pf;
}

struct DkRules {
  using WS = DkWBf16;
  using Args = DkArgs;
  static int bn(int N, int epi) { return dk_bn(N, epi); }
  static constexpr int pf(int BM, int BN) { return dk_pf(BM, BN); }
  template <int BM, int BN, int EPI, bool NORM, int PF>
  static void launch(dim3 grid, const DkArgs& a, hipStream_t s) {
    gemm_dk_kernel<BM, BN, EPI, NORM, PF><<<grid, 256, 0, s>>>(a);
  }
};

// Number of ssq parts a RESID launch of width N writes (the consumer's ssq_parts).
DA_EXPORT int da_gemm_dk_parts(int N) { return (N + dk_bn(N, EPI_RESID) - 1) / dk_bn(N, EPI_RESID); }

// epi: EPI_NONE / EPI_BIAS / EPI_RESID / EPI_SWIGLU. ssq_in (nullable): deferred RMSNorm of A's rows
// over ssq_parts parts (norm over norm_k columns, eps); ssq_out (nullable, EPI_RESID only):
// [da_gemm_dk_parts(N)][64] floats. 1 <= M <= 64, K % 256 == 0, N % 16 == 0 (SwiGLU: N % 32 == 0).
DA_EXPORT int da_gemm_dk(const void* A, int lda, const void* W, void* C, int ldc, const void* bias,
                         const void* resid, int ldr, int M, int N, int K, int epi, const float* ssq_in, int ssq_parts,
                         int norm_k, float eps, float* ssq_out, void* stream) {
  DkArgs a;
  if (!W || !dk_fill(a, 64, A, lda, C, ldc, bias, resid, ldr, M, N, K, epi, ssq_in, ssq_parts, norm_k, eps, ssq_out))
    return (int)hipErrorInvalidValue;
  a.W = (const bf16_t*)W;
  return dk_dispatch<DkRules>(a, epi, (hipStream_t)stream);
}
