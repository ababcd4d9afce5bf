// gemm_dk on fp8 (OCP e4m3) weights with one fp32 scale per weight row: the 2..32-row decode
// products at half the weight bytes of gemm_dk.hip. The kernel is gemm_dk_body.inc on the
// DkWFp8 weight source (gemm_dk.h):
//
//   C[M, N'] = epi( rownorm(A)[M, K] . (Wq[N, K] . s[N])^T )        1 <= M <= 32
//
//  * the codes are streamed with non-temporal 16-B loads (16 codes per lane; a 256-deep k chunk of
//    one weight row is 256 B, 16 lanes), PF chunks in flight per workgroup in a register ring;
//  * on the way into LDS every code is unpacked with v_cvt_pk_f32_fp8 and packed to bf16 (cvt16_bf16,
//    fp8.h; exact). From the LDS store on this IS gemm_dk_kernel: the same swizzled 512-B bf16 rows,
//    the same v_mfma_f32_16x16x32_bf16 sequence per wave (the activations are not quantised, so no
//    fp8 MFMA), the four K quarters summed through LDS in wave order;
//  * the row scale multiplies the finished fp32 sum in the epilogue, before bias / residual / SiLU
//    (SwiGLU: the gate row's and the up row's scale separately). With power-of-two scales the result
//    is therefore bit-identical to gemm_dk on the dequantised bf16 matrix (tests/test_gemm_dk_w8_gpu.py).
//
// The residual producers keep the bf16 kernel's tile width (dk_bn: one part count for both kernels);
// the other epilogues' width and PF differ (dk_w8_bn / dk_w8_pf below): a chunk of BN weight rows is
// half the bytes, the M x K activation block every workgroup re-reads from L2 is not.
#include "gemm_dk.h"

template <int BM, int BN, int EPI, bool NORM, int PF>
__global__ void __launch_bounds__(256)
gemm_dk_w8_kernel(DkW8Args p) {
  using WS = DkWFp8;
#include "gemm_dk_body.inc"
}

// Tile width (BN weight rows) and chunks in flight, from the sweep over the five Phi-3-mini products
// at 4 / 16 / 32 activation rows on an MI355X (bench/w8_dk.py --sweep, profiles/w8dk/README.md; weights
// cold):
//  * width, residual producers (O, down: 3072 weight rows): dk_bn's rule. BN 16 beat BN 32 by 13-25 %
//    and BN 64 by 50-70 %, as at bf16, and one rule keeps one part count (dk_parts) for the bf16 and the
//    fp8 producer of a row-sums buffer.
//  * width, the other epilogues (their width touches no part count): BN 64 from 144 tiles of 64, i.e.
//    from QKV's 9216 weight rows, where dk_bn takes 32: BN 64 was 8 % ahead at 32 activation rows, 2 %
//    at 16, level at 4. 16384 / 32064 weight rows: BN 64 by either rule (first, or within 5 % of BN 32).
//  * PF: the 32- and 64-wide tiles run best with 2 chunks in flight (PF 2 < 4 < 8 on every shape: the
//    ring's registers cost more than the bytes in flight give; PF 1 is slower again), the 16-wide
//    tiles with 4.
static inline int dk_w8_bn(int N, int epi) {
  if (epi != EPI_RESID && N / 64 >= 144) return 64;
  return dk_bn(N, epi);
}

static constexpr int dk_w8_pf(int BN) { return BN == 16 ? 4 : 2; }

struct DkW8Rules {
  using WS = DkWFp8;
  using Args = DkW8Args;
  static int bn(int N, int epi) { return dk_w8_bn(N, epi); }
  static constexpr int pf(int, int BN) { return dk_w8_pf(BN); }
  template <int BM, int BN, int EPI, bool NORM, int PF>
  static void launch(dim3 grid, const DkW8Args& a, hipStream_t s) {
    gemm_dk_w8_kernel<BM, BN, EPI, NORM, PF><<<grid, 256, 0, s>>>(a);
  }
};

// da_gemm_dk with W = Wq (e4m3 bytes, row-major [N, K]) times sw (fp32 [N]) per row. 1 <= M <= 32,
// K % 256 == 0, N % 16 == 0 (SwiGLU: N % 32 == 0); ssq_out: [da_gemm_dk_parts(N)][64] floats
// (a residual producer tiles by dk_bn).
DA_EXPORT int da_gemm_dk_w8(const void* A, int lda, const void* Wq, const void* sw, void* C, int ldc, const void* bias,
                            const void* resid, int ldr, int M, int N, int K, int epi, const float* ssq_in,
                            int ssq_parts, int norm_k, float eps, float* ssq_out, void* stream) {
  DkW8Args a;
  if (!Wq || !sw || !dk_fill(a, 32, A, lda, C, ldc, bias, resid, ldr, M, N, K, epi, ssq_in, ssq_parts, norm_k, eps, ssq_out))
    return (int)hipErrorInvalidValue;
  a.Wq = (const uint8_t*)Wq; a.sw = (const float*)sw;
  return dk_dispatch<DkW8Rules>(a, epi, (hipStream_t)stream);
}

#ifdef DA_GEMM_DK_W8_SWEEP
// Sweep build only (bench/w8_dk.py --build-sweep compiles this file on its own with
// -DDA_GEMM_DK_W8_SWEEP): every tile width / PF arm behind one entry, to pick dk_w8_bn / dk_w8_pf.
// Not part of the kernel library. Arms whose register ring would not fit are refused.
template <int BM, int BN>
static int sweep_pf(const DkW8Args& a, int epi, int pf, hipStream_t s) {
  switch (pf) {
    case 1: return dk_launch_epi<DkW8Rules, BM, BN, 1>(a, epi, s);
    case 2: return dk_launch_epi<DkW8Rules, BM, BN, 2>(a, epi, s);
    case 4: return dk_launch_epi<DkW8Rules, BM, BN, 4>(a, epi, s);
    case 8:
      if constexpr (8 * (BN / 16 + BM / 8) <= 48) return dk_launch_epi<DkW8Rules, BM, BN, 8>(a, epi, s);
      return (int)hipErrorInvalidValue;
    default: return (int)hipErrorInvalidValue;
  }
}

template <int BM>
static int sweep_bn(const DkW8Args& a, int epi, int bn, int pf, hipStream_t s) {
  switch (bn) {
    case 64: return sweep_pf<BM, 64>(a, epi, pf, s);
    case 32: return sweep_pf<BM, 32>(a, epi, pf, s);
    case 16: return sweep_pf<BM, 16>(a, epi, pf, s);
    default: return (int)hipErrorInvalidValue;
  }
}

DA_EXPORT int da_gemm_dk_w8_sweep(const void* A, int lda, const void* Wq, const void* sw, void* C, int ldc,
                                  const void* bias, const void* resid, int ldr, int M, int N, int K, int epi,
                                  const float* ssq_in, int ssq_parts, int norm_k, float eps, float* ssq_out, int bn,
                                  int pf, void* stream) {
  DkW8Args a;
  if (!Wq || !sw || !dk_fill(a, 32, A, lda, C, ldc, bias, resid, ldr, M, N, K, epi, ssq_in, ssq_parts, norm_k, eps, ssq_out))
    return (int)hipErrorInvalidValue;
  a.Wq = (const uint8_t*)Wq; a.sw = (const float*)sw;
  if (M <= 16) return sweep_bn<16>(a, epi, bn, pf, (hipStream_t)stream);
  return sweep_bn<32>(a, epi, bn, pf, (hipStream_t)stream);
}
#endif
