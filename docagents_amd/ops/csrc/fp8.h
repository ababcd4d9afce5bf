// OCP e4m3 (fp8) codes in registers: the conversions and the power-of-two row scale that the fp8
// kernels share. A dword holds 4 codes in memory order; an e4m3 value has 4 significant bits, so
// code -> fp32 -> bf16 is exact.
#pragma once
#include "common.h"

// 4 codes (one dword) -> 4 floats (v_cvt_pk_f32_fp8, two codes per instruction)
__device__ __forceinline__ f32x4_t fp8x4_f32(unsigned w) {
  const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8(w, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8(w, true);
  return f32x4_t{lo[0], lo[1], hi[0], hi[1]};
}

// 8 codes (two dwords) -> 8 bf16: one MFMA A / B fragment
__device__ __forceinline__ bf16x8_t cvt8_bf16(unsigned w0, unsigned w1) {
  const f32x4_t a = fp8x4_f32(w0), b = fp8x4_f32(w1);
  const u32x4_t r = {pack_bf2(a[0], a[1]), pack_bf2(a[2], a[3]), pack_bf2(b[0], b[1]), pack_bf2(b[2], b[3])};
  return __builtin_bit_cast(bf16x8_t, r);
}

// 16 codes -> 16 bf16: lo = codes 0..7, hi = codes 8..15
__device__ __forceinline__ void cvt16_bf16(const u32x4_t& w, u32x4_t& lo, u32x4_t& hi) {
  lo = __builtin_bit_cast(u32x4_t, cvt8_bf16(w[0], w[1]));
  hi = __builtin_bit_cast(u32x4_t, cvt8_bf16(w[2], w[3]));
}

// 4 / 8 floats times inv -> 4 / 8 codes (v_cvt_pk_fp8_f32: round to nearest even, saturating at +-448)
__device__ __forceinline__ unsigned f32x4_fp8(float x0, float x1, float x2, float x3, float inv) {
  int c = __builtin_amdgcn_cvt_pk_fp8_f32(x0 * inv, x1 * inv, 0, false);
  c = __builtin_amdgcn_cvt_pk_fp8_f32(x2 * inv, x3 * inv, c, true);
  return (unsigned)c;
}
__device__ __forceinline__ u32x2_t f32x8_fp8(const float (&v)[8], float inv) {
  return u32x2_t{f32x4_fp8(v[0], v[1], v[2], v[3], inv), f32x4_fp8(v[4], v[5], v[6], v[7], inv)};
}

// The power-of-two row scale of the fp8 KV cache, the fp8 index and quant_weight_fp8_pow2: sc = the
// smallest 2^e with amax / 2^e <= 448 (1 for an all-zero row), inv = 2^-e. code * sc is exact in bf16.
__device__ __forceinline__ void fp8_pow2_scale(float amax, float& sc, float& inv) {
  // 448 = 1.75 * 2^8: amax = f * 2^E, f in [1, 2) -> e = E - 8 (+ 1 if f > 1.75)
  const unsigned ab = __float_as_uint(amax);
  int e = (int)(ab >> 23) - 127 - 8 + ((ab & 0x7fffffu) > 0x600000u ? 1 : 0);
  e = max(e, -126);
  if (amax == 0.f) e = 0;
  sc = __uint_as_float((unsigned)(127 + e) << 23);
  inv = __uint_as_float((unsigned)(127 - e) << 23);
}
