// What gemm_dk.hip (bf16 weights) and gemm_dk_w8.hip (e4m3 weights with a scale per row) share: the
// weight sources, the launch dispatch and the argument checks. The kernel body itself is
// gemm_dk_body.inc, included inside each __global__ kernel after `using WS = <weight source>;`. A
// weight source (DkWBf16 / DkWFp8) says how a chunk of W rows gets from global memory into the
// swizzled bf16 LDS rows and which row scales the finished sums take; everything else is one body.
// (The body is text, not an inlined function: with this compiler the same statements inside a
// __forceinline__ function called from the kernel allocate the prefetch ring differently and change
// the register counts of a third of the instances.)
#pragma once
#include "fp8.h"
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

struct DkW8Args : DkArgs {  // W unused
  const uint8_t* Wq;        // [N, K] e4m3 codes
  const float* sw;          // [N] row scales
};

// Output-tile width: the widest of 64 / 32 / 16 W rows that still gives >= 192 workgroups (SwiGLU
// needs whole 32-row gate/up groups).
static inline int dk_bn(int N, int epi) {
  if (N / 64 >= 192) return 64;
  if (N / 32 >= 192 || epi == EPI_SWIGLU) return 32;
  return 16;
}

// ---- weight sources: piece i (16 B) of thread tid for the BN x 256 chunk of W at (n0, k0) ----
// The staged rows are 512 B of bf16; 16-B chunk ch of row r sits at slot ch ^ (r & 15): the 16 rows
// one ds_read_b128 lane group reads (same chunk) land on 16 distinct slots of a 256-B bank row.
__device__ __forceinline__ char* dk_slot(char* rows, int r, int ch) { return rows + r * 512 + ((ch ^ (r & 15)) << 4); }

struct DkWBf16 {  // 32 pieces of 8 bf16 per row, whole 512-B row segments
  using Args = DkArgs;
  static constexpr bool kScaled = false;  // no row scales: scales8 is empty, the sums are not multiplied
  static constexpr bool kRowBlocks = true;  // 33..64 rows: two row blocks per n-tile (p.rb == 2)
  static constexpr int lw(int BN) { return BN / 8; }
  static __device__ __forceinline__ u32x4_t load(const Args& p, int i, int tid, int n0, int k0) {
    const int idx = tid + 256 * i, r = idx >> 5, ch = idx & 31;
    return __builtin_nontemporal_load((const u32x4_t*)(p.W + (size_t)min(n0 + r, p.N - 1) * p.K + k0 + ch * 8));
  }
  static __device__ __forceinline__ void store(char* sw, int i, int tid, const u32x4_t& x) {
    const int idx = tid + 256 * i, r = idx >> 5, ch = idx & 31;
    *(u32x4_t*)dk_slot(sw, r, ch) = x;
  }
  static __device__ __forceinline__ void scales8(const Args&, int, float (&)[8]) {}
};

struct DkWFp8 {  // 16 pieces of 16 codes per row; a piece becomes the bf16 chunks 2 ch8, 2 ch8 + 1
  using Args = DkW8Args;
  static constexpr bool kScaled = true;      // p.sw[n] multiplies the finished fp32 sum of column n
  static constexpr bool kRowBlocks = false;  // M <= 32
  static constexpr int lw(int BN) { return BN / 16; }
  static __device__ __forceinline__ u32x4_t load(const Args& p, int i, int tid, int n0, int k0) {
    const int idx = tid + 256 * i, r = idx >> 4, ch8 = idx & 15;
    return __builtin_nontemporal_load((const u32x4_t*)(p.Wq + (size_t)min(n0 + r, p.N - 1) * p.K + k0 + ch8 * 16));
  }
  static __device__ __forceinline__ void store(char* sw, int i, int tid, const u32x4_t& x) {
    const int idx = tid + 256 * i, r = idx >> 4, ch8 = idx & 15;
    u32x4_t lo, hi;
    cvt16_bf16(x, lo, hi);
    *(u32x4_t*)dk_slot(sw, r, 2 * ch8) = lo;
    *(u32x4_t*)dk_slot(sw, r, 2 * ch8 + 1) = hi;
  }
  // the 8 row scales from weight row n on (n % 8 == 0; rows past N: never stored, scale 1)
  static __device__ __forceinline__ void scales8(const Args& p, int n, float (&s)[8]) {
    const bool in = n < p.N;
    const f32x4_t s0 = in ? *(const f32x4_t*)(p.sw + n) : f32x4_t{1.f, 1.f, 1.f, 1.f};
    const f32x4_t s1 = in ? *(const f32x4_t*)(p.sw + n + 4) : f32x4_t{1.f, 1.f, 1.f, 1.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) { s[e] = s0[e]; s[4 + e] = s1[e]; }
  }
};

// ---- host: BM x BN x EPI x NORM dispatch. R (next to each __global__ kernel) gives the weight source WS,
// the kernel's Args, the tile-width rule bn(N, epi), the chunks in flight pf(BM, BN) and
// launch<BM, BN, EPI, NORM, PF>(grid, args, stream).
template <class R, int BM, int BN, int EPI, bool NORM, int PF>
static int dk_launch(const typename R::Args& a, hipStream_t s) {
  const int nt = (a.N + BN - 1) / BN;
  // row blocks: pairs of workgroups i, i + 8 per n-tile, the grid padded to whole groups of 16
  const bool rb2 = R::WS::kRowBlocks && a.rb == 2;
  R::template launch<BM, BN, EPI, NORM, PF>(dim3(rb2 ? (nt + 7) / 8 * 16 : nt), a, s);
  return (int)hipGetLastError();
}

template <class R, int BM, int BN, int PF>
static int dk_launch_epi(const typename R::Args& a, int epi, hipStream_t s) {
  const bool norm = a.ssq_in != nullptr;
  switch (epi) {
    case EPI_NONE: case EPI_BIAS:
      return norm ? dk_launch<R, BM, BN, EPI_NONE, true, PF>(a, s) : dk_launch<R, BM, BN, EPI_NONE, false, PF>(a, s);
    case EPI_RESID:  // the residual producers never take a deferred norm
      return norm ? (int)hipErrorInvalidValue : dk_launch<R, BM, BN, EPI_RESID, false, PF>(a, s);
    case EPI_SWIGLU:
      if constexpr (BN >= 32)
        return norm ? dk_launch<R, BM, BN, EPI_SWIGLU, true, PF>(a, s)
                    : dk_launch<R, BM, BN, EPI_SWIGLU, false, PF>(a, s);
      return (int)hipErrorInvalidValue;
    default: return (int)hipErrorInvalidValue;
  }
}

template <class R, int BM>
static int dk_launch_bn(const typename R::Args& a, int epi, hipStream_t s) {
  switch (R::bn(a.N, epi)) {
    case 64: return dk_launch_epi<R, BM, 64, R::pf(BM, 64)>(a, epi, s);
    case 32: return dk_launch_epi<R, BM, 32, R::pf(BM, 32)>(a, epi, s);
    default: return dk_launch_epi<R, BM, 16, R::pf(BM, 16)>(a, epi, s);
  }
}

// 33..64 rows (a.rb == 2): two 32-row blocks per n-tile (less A re-read per W byte than one 64-row block)
template <class R>
static int dk_dispatch(const typename R::Args& a, int epi, hipStream_t s) {
  return a.M <= 16 ? dk_launch_bn<R, 16>(a, epi, s) : dk_launch_bn<R, 32>(a, epi, s);
}

// Checks everything the body relies on and fills the arguments, the weight pointers excepted (the
// caller's: W, or Wq and sw). false: refused. 1 <= M <= max_m (64, or 32 without row blocks),
// K % 256 == 0, N % 16 == 0 (SwiGLU: N % 32 == 0); rows, bias and the row-sum buffers are read and
// written 16 B at a time.
static inline bool dk_fill(DkArgs& a, int max_m, const void* A, int lda, void* C, int ldc, const void* bias,
                           const void* resid, int ldr, int M, int N, int K, int epi, const float* ssq_in,
                           int ssq_parts, int norm_k, float eps, float* ssq_out) {
  if (M < 1 || M > max_m || N < 16 || K < 256 || K % 256 || N % 16 || lda % 8 || ldc % 8 || lda < K) return false;
  if (!A || !C) return false;
  if (epi != EPI_NONE && epi != EPI_BIAS && epi != EPI_RESID && epi != EPI_SWIGLU) return false;
  if (epi == EPI_SWIGLU && N % 32) return false;
  if (ldc < (epi == EPI_SWIGLU ? N / 2 : N)) return false;
  if (epi == EPI_RESID && (!resid || ldr % 8 || ldr < N)) return false;
  if (ssq_out && epi != EPI_RESID) return false;
  if (ssq_in && (epi == EPI_RESID || ssq_parts < 1 || norm_k < 1 || !(eps > 0.f))) return false;
  a = DkArgs{};
  a.A = (const bf16_t*)A; a.C = (bf16_t*)C;
  a.bias = (const bf16_t*)bias; a.resid = (const bf16_t*)resid;
  a.ssq_in = ssq_in; a.ssq_out = ssq_out;
  a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldc = ldc; a.ldr = ldr;
  a.ssq_parts = ssq_parts; a.norm_k = norm_k; a.eps = eps;
  a.rb = M > 32 ? 2 : 1;
  return true;
}
