// OCP MXFP4 in registers: e2m1 codes (two per byte: element 2j in bits 3:0 of byte j, element 2j+1 in
// bits 7:4) and one e8m0 power-of-two scale byte per 32 consecutive elements. An e2m1 value has 2
// significant bits, so code * 2^e -> fp32 -> bf16 is exact.
#pragma once
#include "common.h"

// e8m0 scale byte -> 2^(b - 127). quant_weight_mxfp4 stores bytes 1..254 only (never 0, never the
// e8m0 NaN 255), so b << 23 is a normal float.
__device__ __forceinline__ float e8m0_f32(unsigned b) { return __uint_as_float(b << 23); }

// 8 codes (one dword, memory order) times scale -> 8 floats (v_cvt_scalef32_pk_f32_fp4: one byte =
// two codes per instruction, the product with the scale is part of the conversion and exact for a
// power of two; the byte selector is an immediate)
__device__ __forceinline__ void fp4x8_f32(unsigned w, float scale, float (&f)[8]) {
  const f32x2_t b0 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, scale, 0);
  const f32x2_t b1 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, scale, 1);
  const f32x2_t b2 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, scale, 2);
  const f32x2_t b3 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, scale, 3);
  f[0] = b0[0]; f[1] = b0[1]; f[2] = b1[0]; f[3] = b1[1];
  f[4] = b2[0]; f[5] = b2[1]; f[6] = b3[0]; f[7] = b3[1];
}
