// What the two gemm_dk kernels share: gemm_dk.hip (bf16 weights) and gemm_dk_w8.hip (e4m3 weights).
#pragma once
#include "gemm.h"

struct DkArgs {
  const bf16_t* A; const bf16_t* W; bf16_t* C;
  const bf16_t* bias; const bf16_t* resid;
  const float* ssq_in;  // NORM: [ssq_parts][64] partial sums of squares of A's rows
  float* ssq_out;       // EPI_RESID (nullable): [gridDim.x][64] sums of squares of this tile's output rows
  int M, N, K, lda, ldc, ldr, ssq_parts, norm_k;
  float eps;
  int rb;  // row blocks of BM rows: 1, or 2 (M > BM; workgroup pairs share an XCD)
};

// Output-tile width: the widest of 64 / 32 / 16 W rows that still gives >= 192 workgroups (SwiGLU
// needs whole 32-row gate/up groups).
static inline int dk_bn(int N, int epi) {
  if (N / 64 >= 192) return 64;
  if (N / 32 >= 192 || epi == EPI_SWIGLU) return 32;
  return 16;
}
