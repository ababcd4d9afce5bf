// The weight-streaming decode tiles of gemm.hip on fp8 (OCP e4m3) weights with one fp32 scale per
// weight row: the 33..128-row decode products at half the weight bytes.
//
//   C[M, N'] = epi( A[M, K] . (Wq[N, K] . s[N])^T )        1 <= M <= 128
//
// The kernel is gemm_tile_body.inc with W8 set, for the two tiles those rows run on: 64x128 (tile 2,
// 1x4 waves) and 128x64 (tile 9, 2x2 waves), 4 k-tiles in flight each.
//  * A is staged as in gemm_bf16_kernel (bf16, 16-B loads, the same swizzled LDS rows);
//  * the codes are streamed with 16-B loads (16 codes per lane: a 64-deep k-tile of one weight row
//    is 64 B, 4 lanes) and unpacked with v_cvt_pk_f32_fp8 + a bf16 pack on the way into LDS (exact);
//  * from LDS on this IS gemm_bf16_kernel: the same v_mfma_f32_16x16x32_bf16 sequence, K order and
//    split-K layout (the activations are not quantised, so no fp8 MFMA);
//  * the row scale multiplies the fp32 value of its column before anything else in the epilogue,
//    EPI_PARTIAL included, so the split-K reduces of gemm.hip run unchanged on these partials. With
//    power-of-two scales the result is bit-identical to the bf16 kernel on the dequantised matrix
//    (tests/test_gemm_tile_w8_gpu.py).
//
// The entry points (da_gemm_tile_w8, da_gemm_dk_splitk_w8, da_gemm_resid_rmsnorm_w8) sit next to the
// reduce kernels in gemm.hip and launch the tiles through launch_gemm_tile_w8.
#include "fp8.h"
#include "gemm.h"

template <int BM, int BN, int WM, int WN, int EPI, int PF, bool NT>
__global__ void __launch_bounds__(256)
gemm_tile_w8_kernel(GemmArgs p) {
  constexpr bool W8 = true, W_NT = NT;
#include "gemm_tile_body.inc"
}

// Non-temporal code loads, per tile, from the A/B on the five Phi-3-mini products at 40 / 64 / 96 / 128
// rows (bench/w8_mid.py --nt, profiles/w8mid/README.md): default loads on both tiles. 64x128: a k-tile of
// one weight row is half a 128-B line and the next k-tile's load wants the other half from L2 (and above
// 64 rows two row blocks share the tile): non-temporal lost on every product, up to 30 % (LM head).
// 128x64: level on O, 2-5 % slower on down (K = 8192). -1: that rule; 0 / 1: every tile without / with (the A/B switch, da_gemm_tile_w8_nt).
static int g_nt = -1;

DA_EXPORT int da_gemm_tile_w8_nt(int v) {
  if (v >= -1 && v <= 1) g_nt = v;
  return g_nt;
}


template <int BM, int BN, int WM, int WN, bool NT>
static int launch_w8(const GemmArgs& a, int epi, int splits, hipStream_t s) {
  const int ntm = (a.M + BM - 1) / BM, ntn = (a.N + BN - 1) / BN;
  dim3 grid(ntm * ntn, 1, splits), block(256);
  switch (splits > 1 ? (int)EPI_PARTIAL : epi) {
    case EPI_NONE: gemm_tile_w8_kernel<BM, BN, WM, WN, EPI_NONE, 4, NT><<<grid, block, 0, s>>>(a); break;
    case EPI_BIAS: gemm_tile_w8_kernel<BM, BN, WM, WN, EPI_BIAS, 4, NT><<<grid, block, 0, s>>>(a); break;
    case EPI_SWIGLU: gemm_tile_w8_kernel<BM, BN, WM, WN, EPI_SWIGLU, 4, NT><<<grid, block, 0, s>>>(a); break;
    case EPI_RESID: gemm_tile_w8_kernel<BM, BN, WM, WN, EPI_RESID, 4, NT><<<grid, block, 0, s>>>(a); break;
    case EPI_PARTIAL: gemm_tile_w8_kernel<BM, BN, WM, WN, EPI_PARTIAL, 4, NT><<<grid, block, 0, s>>>(a); break;
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

int launch_gemm_tile_w8(const GemmArgs& a, int tile, int epi, int splits, hipStream_t s) {
  if (!a.W || !a.sw || a.M < 1 || a.M > 128 || a.K < 64 || a.K % 64 || a.N < 8 || a.N % 8) return (int)hipErrorInvalidValue;
  const bool nt = g_nt == 1;
  if (tile == 2) return nt ? launch_w8<64, 128, 1, 4, true>(a, epi, splits, s) : launch_w8<64, 128, 1, 4, false>(a, epi, splits, s);
  if (tile == 9) return nt ? launch_w8<128, 64, 2, 2, true>(a, epi, splits, s) : launch_w8<128, 64, 2, 2, false>(a, epi, splits, s);
  return (int)hipErrorInvalidValue;
}
