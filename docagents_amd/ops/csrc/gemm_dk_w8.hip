// gemm_dk on fp8 (OCP e4m3) weights with one fp32 scale per weight row: the 2..32-row decode
// products at half the weight bytes of gemm_dk.hip, whose structure this keeps.
//
//   C[M, N'] = epi( rownorm(A)[M, K] . (Wq[N, K] . s[N])^T )        1 <= M <= 32
//
//  * the codes are streamed with non-temporal 16-B loads (16 codes per lane; a 256-deep k chunk of
//    one weight row is 256 B, 16 lanes), PF chunks in flight per workgroup in a register ring;
//  * on the way into LDS every code is unpacked with v_cvt_pk_f32_fp8 and packed to bf16 (exact: an
//    e4m3 value has 4 significant bits). From the LDS store on this IS gemm_dk_kernel: the same
//    swizzled 512-B bf16 rows, the same v_mfma_f32_16x16x32_bf16 sequence per wave (the activations
//    are not quantised, so no fp8 MFMA), the four K quarters summed through LDS in wave order;
//  * the row scale multiplies the finished fp32 sum in the epilogue, before bias / residual / SiLU
//    (SwiGLU: the gate row's and the up row's scale separately). With power-of-two scales the result
//    is therefore bit-identical to gemm_dk on the dequantised bf16 matrix (tests/test_gemm_dk_w8_gpu.py).
//
// The residual producers keep the bf16 kernel's tile width (dk_bn: one part count for both kernels);
// the other epilogues' width and PF differ (dk_w8_bn / dk_w8_pf below): a chunk of BN weight rows is
// half the bytes, the M x K activation block every workgroup re-reads from L2 is not.
#include "gemm_dk.h"

struct DkW8Args {
  DkArgs d;            // d.W unused
  const uint8_t* Wq;   // [N, K] e4m3 codes
  const float* sw;     // [N] row scales
};

template <int BM, int BN, int EPI, bool NORM, int PF>
__global__ void __launch_bounds__(256)
gemm_dk_w8_kernel(DkW8Args pa) {
  const DkArgs& p = pa.d;
  constexpr int FM = BM / 16, FN = BN / 16;
  constexpr int KC = 256;                      // k per chunk: one 64-deep k-tile per wave
  constexpr int ROWB = KC * 2;                 // 512 B per staged (bf16) row
  constexpr int LW = BN / 16, LA = BM / 8;     // 16-B pieces per thread per chunk (W: 16 per row, A: 32)
  constexpr int CHUNK = (BN + BM) * ROWB;
  constexpr int SLD = BN + 4;
  constexpr int RED = 4 * BM * SLD * 4;
  constexpr int LDS_BYTES = 2 * CHUNK > RED ? 2 * CHUNK : RED;
  __shared__ __attribute__((aligned(16))) char smem[LDS_BYTES];
  __shared__ float sinv[BM];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const int tile = blockIdx.x;
  const int n0 = tile * BN;
  if (n0 >= p.N) return;
  const int Mb = min(BM, p.M);
  const int nch = p.K / KC;
  const int kl = nch - 1;

  // ---- global -> registers: whole row segments (W: 16 lanes x 16 B of codes, A: 32 lanes x 16 B) ----
  u32x4_t rw[PF][LW], ra[PF][LA];
  auto gload = [&](u32x4_t (&xw)[LW], u32x4_t (&xa)[LA], int c) {
    const int k0 = c * KC;
#pragma unroll
    for (int i = 0; i < LW; ++i) {
      const int idx = tid + 256 * i, r = idx >> 4, ch = idx & 15;
      xw[i] = __builtin_nontemporal_load((const u32x4_t*)(pa.Wq + (size_t)min(n0 + r, p.N - 1) * p.K + k0 + ch * 16));
    }
#pragma unroll
    for (int i = 0; i < LA; ++i) {
      const int idx = tid + 256 * i, r = idx >> 5, ch = idx & 31;
      xa[i] = *(const u32x4_t*)(p.A + (size_t)min(r, Mb - 1) * p.lda + k0 + ch * 8);
    }
  };
  // LDS rows of 512 B (bf16); 16-B chunk ch of row r at slot ch ^ (r & 15), as gemm_dk_kernel. A piece
  // of 16 codes becomes the two bf16 chunks 2 ch8, 2 ch8 + 1 of its row.
  auto lstore = [&](const u32x4_t (&xw)[LW], const u32x4_t (&xa)[LA], int buf) {
    char* sw = smem + buf * CHUNK;
    char* sa = sw + BN * ROWB;
#pragma unroll
    for (int i = 0; i < LW; ++i) {
      const int idx = tid + 256 * i, r = idx >> 4, ch8 = idx & 15;
      unsigned b[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {  // word e = codes 4e .. 4e+3
        const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8(xw[i][e], false);
        const f32x2_t hi = __builtin_amdgcn_cvt_pk_f32_fp8(xw[i][e], true);
        b[2 * e] = pack_bf2(lo[0], lo[1]);
        b[2 * e + 1] = pack_bf2(hi[0], hi[1]);
      }
      *(u32x4_t*)(sw + r * ROWB + (((2 * ch8) ^ (r & 15)) << 4)) = u32x4_t{b[0], b[1], b[2], b[3]};
      *(u32x4_t*)(sw + r * ROWB + (((2 * ch8 + 1) ^ (r & 15)) << 4)) = u32x4_t{b[4], b[5], b[6], b[7]};
    }
#pragma unroll
    for (int i = 0; i < LA; ++i) {
      const int idx = tid + 256 * i, r = idx >> 5, ch = idx & 31;
      *(u32x4_t*)(sa + r * ROWB + ((ch ^ (r & 15)) << 4)) = xa[i];
    }
  };

#pragma unroll
  for (int u = 0; u < PF; ++u) {
    gload(rw[u], ra[u], min(u, kl));
    asm volatile("" ::: "memory");  // issue order = chunk order (counted waits)
  }
  // ---- deferred RMSNorm: inv[m] from the producer's per-part sums (fixed summation order) ----
  if constexpr (NORM) {
    constexpr int RQ = BM / 4, PL = 256 / RQ;
    __shared__ f32x4_t sq4[PL][RQ];
    const int rq = tid % RQ, pl = tid / RQ;
    f32x4_t a4{0.f, 0.f, 0.f, 0.f};
    for (int q0 = pl; q0 < p.ssq_parts; q0 += 8 * PL) {  // 8 parts' loads issued before their adds
      f32x4_t v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        v[j] = *(const f32x4_t*)(p.ssq_in + (size_t)min(q0 + j * PL, p.ssq_parts - 1) * 64 + 4 * rq);
#pragma unroll
      for (int j = 0; j < 8; ++j) a4 += (q0 + j * PL < p.ssq_parts) ? v[j] : f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
    sq4[pl][rq] = a4;
    __syncthreads();
    if (tid < BM) {
      float ss = 0.f;
      for (int q = 0; q < PL; ++q) ss += sq4[q][tid >> 2][tid & 3];
      sinv[tid] = rsqrtf(ss / p.norm_k + p.eps);
    }
  }
  lstore(rw[0], ra[0], 0);
  __syncthreads();
  float inv[FM];
#pragma unroll
  for (int i = 0; i < FM; ++i) inv[i] = NORM ? sinv[min(16 * i + fr, Mb - 1)] : 1.f;

  f32x4_t acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  for (int c0 = 0; c0 < nch; c0 += PF) {
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      const int c = c0 + u;
      const int cur = c & 1;
      // slot u held chunk c, already in LDS: refill it PF chunks ahead (clamped, branch-free)
      if (PF > 1 || c + 1 < nch) gload(rw[u], ra[u], min(c + PF, kl));
      if (c >= nch) continue;
      const char* sw = smem + cur * CHUNK;
      const char* sa = sw + BN * ROWB;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int ch = 8 * w + 4 * kk + fg;  // this wave's k-tile of the chunk
        bf16x8_t af[FM], bfr[FN];
#pragma unroll
        for (int i = 0; i < FM; ++i) {
          const int r = 16 * i + fr;
          af[i] = *(const bf16x8_t*)(sa + r * ROWB + ((ch ^ (r & 15)) << 4));
          if constexpr (NORM) {
            bf16x8_t y;
#pragma unroll
            for (int e = 0; e < 8; e += 2) {
              const unsigned pk = pack_bf2(bf2f((bf16_t)af[i][e]) * inv[i], bf2f((bf16_t)af[i][e + 1]) * inv[i]);
              y[e] = (short)(pk & 0xffff);
              y[e + 1] = (short)(pk >> 16);
            }
            af[i] = y;
          }
        }
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          const int r = 16 * j + fr;
          bfr[j] = *(const bf16x8_t*)(sw + r * ROWB + ((ch ^ (r & 15)) << 4));
        }
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
          for (int j = 0; j < FN; ++j) acc[i][j] = mfma16(af[i], bfr[j], acc[i][j]);
      }
      if (c + 1 < nch) lstore(rw[(u + 1) % PF], ra[(u + 1) % PF], cur ^ 1);
      // LDS writes visible + buffer reads done; a raw barrier (a __syncthreads() fence would drain
      // vmcnt and cancel the PF - 1 chunks in flight)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
  }
  float (*red)[BM][SLD] = (float (*)[BM][SLD])smem;  // the staging buffers are free now

  // ---- the four K quarters -> one tile, in wave order (deterministic) ----
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) red[w][16 * i + 4 * fg + q][16 * j + fr] = acc[i][j][q];
  __syncthreads();

  constexpr int BNO = EPI == EPI_SWIGLU ? BN / 2 : BN;  // output columns of the tile
  constexpr int CPR = BNO / 8;                          // 16-B output chunks per row
  static_assert(CPR >= 1 && 256 % CPR == 0, "tile");
  // the 8 row scales from weight row n on (n % 8 == 0; rows past N: never stored, scale 1)
  auto scales8 = [&](int n, float (&s)[8]) {
    const bool in = n < p.N;
    const f32x4_t s0 = in ? *(const f32x4_t*)(pa.sw + n) : f32x4_t{1.f, 1.f, 1.f, 1.f};
    const f32x4_t s1 = in ? *(const f32x4_t*)(pa.sw + n + 4) : f32x4_t{1.f, 1.f, 1.f, 1.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) { s[e] = s0[e]; s[4 + e] = s1[e]; }
  };
  for (int t = tid; t < BM * CPR; t += 256) {
    const int m = t / CPR, ch = t % CPR;
    float v[8];
    if constexpr (EPI == EPI_SWIGLU) {
      const int g = ch >> 1, hh = ch & 1;
      const int gc = 32 * g + 8 * hh;
      float sg[8], su[8];
      scales8(n0 + gc, sg);
      scales8(n0 + gc + 16, su);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float gt = red[0][m][gc + e] + red[1][m][gc + e] + red[2][m][gc + e] + red[3][m][gc + e];
        const float up = red[0][m][gc + 16 + e] + red[1][m][gc + 16 + e] + red[2][m][gc + 16 + e] +
                         red[3][m][gc + 16 + e];
        v[e] = silu(gt * sg[e]) * (up * su[e]);
      }
      const int oc = n0 / 2 + 16 * g + 8 * hh;
      if (m < Mb && oc < p.N / 2) {  // a ragged last tile (N % BN == 32) holds one gate/up group
        *(u32x4_t*)(p.C + (size_t)m * p.ldc + oc) =
            u32x4_t{pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]), pack_bf2(v[4], v[5]), pack_bf2(v[6], v[7])};
      }
    } else {
      const int c = 8 * ch;
      const int gn = n0 + c;
      const bool ok = m < Mb && gn < p.N;
      float sc[8];
      scales8(gn, sc);
#pragma unroll
      for (int e = 0; e < 8; ++e)
        v[e] = (red[0][m][c + e] + red[1][m][c + e] + red[2][m][c + e] + red[3][m][c + e]) * sc[e];
      if (p.bias && ok) {
        const u32x4_t b = *(const u32x4_t*)(p.bias + gn);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[2 * e] += bf2f((bf16_t)(b[e] & 0xffff));
          v[2 * e + 1] += bf2f((bf16_t)(b[e] >> 16));
        }
      }
      if constexpr (EPI == EPI_RESID) {
        if (ok) {
          const u32x4_t r = *(const u32x4_t*)(p.resid + (size_t)m * p.ldr + gn);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            v[2 * e] += bf2f((bf16_t)(r[e] & 0xffff));
            v[2 * e + 1] += bf2f((bf16_t)(r[e] >> 16));
          }
        }
      }
      const u32x4_t o{pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]), pack_bf2(v[4], v[5]), pack_bf2(v[6], v[7])};
      if (ok) *(u32x4_t*)(p.C + (size_t)m * p.ldc + gn) = o;
      if constexpr (EPI == EPI_RESID) {
        if (p.ssq_out) {  // sum of squares of the bf16 values the stream now holds
          float sq = 0.f;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float lo = bf2f((bf16_t)(o[e] & 0xffff)), hi = bf2f((bf16_t)(o[e] >> 16));
            sq += lo * lo + hi * hi;
          }
          if (!ok) sq = 0.f;
#pragma unroll
          for (int x = 1; x < CPR; x <<= 1) sq += __shfl_xor(sq, x, 64);
          if (ch == 0) p.ssq_out[(size_t)tile * 64 + m] = sq;
        }
      }
    }
  }
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

template <int BM, int BN, int EPI, bool NORM, int PF>
static int dkw8_launch5(const DkW8Args& a, hipStream_t s) {
  dim3 grid((a.d.N + BN - 1) / BN), block(256);
  gemm_dk_w8_kernel<BM, BN, EPI, NORM, PF><<<grid, block, 0, s>>>(a);
  return (int)hipGetLastError();
}

template <int BM, int BN, int EPI, int PF>
static int dkw8_launch3(const DkW8Args& a, bool norm, hipStream_t s) {
  if constexpr (EPI == EPI_RESID) {  // the residual producers never take a deferred norm
    return norm ? (int)hipErrorInvalidValue : dkw8_launch5<BM, BN, EPI, false, PF>(a, s);
  } else {
    return norm ? dkw8_launch5<BM, BN, EPI, true, PF>(a, s) : dkw8_launch5<BM, BN, EPI, false, PF>(a, s);
  }
}

template <int BM, int BN, int PF>
static int dkw8_launch2(const DkW8Args& a, int epi, bool norm, hipStream_t s) {
  switch (epi) {
    case EPI_NONE: case EPI_BIAS: return dkw8_launch3<BM, BN, EPI_NONE, PF>(a, norm, s);
    case EPI_RESID: return dkw8_launch3<BM, BN, EPI_RESID, PF>(a, norm, s);
    case EPI_SWIGLU:
      if constexpr (BN >= 32) return dkw8_launch3<BM, BN, EPI_SWIGLU, PF>(a, norm, s);
      return (int)hipErrorInvalidValue;
    default: return (int)hipErrorInvalidValue;
  }
}

template <int BM>
static int dkw8_launch1(const DkW8Args& a, int epi, bool norm, hipStream_t s) {
  switch (dk_w8_bn(a.d.N, epi)) {
    case 64: return dkw8_launch2<BM, 64, dk_w8_pf(64)>(a, epi, norm, s);
    case 32: return dkw8_launch2<BM, 32, dk_w8_pf(32)>(a, epi, norm, s);
    default: return dkw8_launch2<BM, 16, dk_w8_pf(16)>(a, epi, norm, s);
  }
}

static bool dk_w8_fill(DkW8Args& a, const void* A, int lda, const void* Wq, const void* sw, void* C, int ldc,
                       const void* bias, const void* resid, int ldr, int M, int N, int K, int epi, const float* ssq_in,
                       int ssq_parts, int norm_k, float eps, float* ssq_out) {
  if (M < 1 || M > 32 || N < 16 || K < 256 || K % 256 || N % 16 || lda % 8 || ldc % 8 || lda < K) return false;
  if (!A || !Wq || !sw || !C) return false;
  if (epi != EPI_NONE && epi != EPI_BIAS && epi != EPI_RESID && epi != EPI_SWIGLU) return false;
  if (epi == EPI_SWIGLU && N % 32) return false;
  if (ldc < (epi == EPI_SWIGLU ? N / 2 : N)) return false;
  if (epi == EPI_RESID && (!resid || ldr % 8 || ldr < N)) return false;
  if (ssq_out && epi != EPI_RESID) return false;
  if (ssq_in && (epi == EPI_RESID || ssq_parts < 1 || norm_k < 1 || !(eps > 0.f))) return false;
  a = DkW8Args{};
  a.d.A = (const bf16_t*)A; a.d.C = (bf16_t*)C;
  a.d.bias = (const bf16_t*)bias; a.d.resid = (const bf16_t*)resid;
  a.d.ssq_in = ssq_in; a.d.ssq_out = ssq_out;
  a.d.M = M; a.d.N = N; a.d.K = K; a.d.lda = lda; a.d.ldc = ldc; a.d.ldr = ldr;
  a.d.ssq_parts = ssq_parts; a.d.norm_k = norm_k; a.d.eps = eps; a.d.rb = 1;
  a.Wq = (const uint8_t*)Wq; a.sw = (const float*)sw;
  return true;
}

// da_gemm_dk with W = Wq (e4m3 bytes, row-major [N, K]) times sw (fp32 [N]) per row. 1 <= M <= 32,
// K % 256 == 0, N % 16 == 0 (SwiGLU: N % 32 == 0); ssq_out: [da_gemm_dk_parts(N)][64] floats
// (a residual producer tiles by dk_bn).
DA_EXPORT int da_gemm_dk_w8(const void* A, int lda, const void* Wq, const void* sw, void* C, int ldc, const void* bias,
                            const void* resid, int ldr, int M, int N, int K, int epi, const float* ssq_in,
                            int ssq_parts, int norm_k, float eps, float* ssq_out, void* stream) {
  DkW8Args a;
  if (!dk_w8_fill(a, A, lda, Wq, sw, C, ldc, bias, resid, ldr, M, N, K, epi, ssq_in, ssq_parts, norm_k, eps, ssq_out))
    return (int)hipErrorInvalidValue;
  const bool norm = ssq_in != nullptr;
  if (M <= 16) return dkw8_launch1<16>(a, epi, norm, (hipStream_t)stream);
  return dkw8_launch1<32>(a, epi, norm, (hipStream_t)stream);
}

#ifdef DA_GEMM_DK_W8_SWEEP
// Sweep build only (bench/w8_dk.py --build-sweep compiles this file on its own with
// -DDA_GEMM_DK_W8_SWEEP): every tile width / PF arm behind one entry, to pick dk_w8_bn / dk_w8_pf.
// Not part of the kernel library. Arms whose register ring would not fit are refused.
template <int BM, int BN>
static int sweep_pf(const DkW8Args& a, int epi, bool norm, int pf, hipStream_t s) {
  switch (pf) {
    case 1: return dkw8_launch2<BM, BN, 1>(a, epi, norm, s);
    case 2: return dkw8_launch2<BM, BN, 2>(a, epi, norm, s);
    case 4: return dkw8_launch2<BM, BN, 4>(a, epi, norm, s);
    case 8:
      if constexpr (8 * (BN / 16 + BM / 8) <= 48) return dkw8_launch2<BM, BN, 8>(a, epi, norm, s);
      return (int)hipErrorInvalidValue;
    default: return (int)hipErrorInvalidValue;
  }
}

template <int BM>
static int sweep_bn(const DkW8Args& a, int epi, bool norm, int bn, int pf, hipStream_t s) {
  switch (bn) {
    case 64: return sweep_pf<BM, 64>(a, epi, norm, pf, s);
    case 32: return sweep_pf<BM, 32>(a, epi, norm, pf, s);
    case 16: return sweep_pf<BM, 16>(a, epi, norm, pf, s);
    default: return (int)hipErrorInvalidValue;
  }
}

DA_EXPORT int da_gemm_dk_w8_sweep(const void* A, int lda, const void* Wq, const void* sw, void* C, int ldc,
                                  const void* bias, const void* resid, int ldr, int M, int N, int K, int epi,
                                  const float* ssq_in, int ssq_parts, int norm_k, float eps, float* ssq_out, int bn,
                                  int pf, void* stream) {
  DkW8Args a;
  if (!dk_w8_fill(a, A, lda, Wq, sw, C, ldc, bias, resid, ldr, M, N, K, epi, ssq_in, ssq_parts, norm_k, eps, ssq_out))
    return (int)hipErrorInvalidValue;
  const bool norm = ssq_in != nullptr;
  if (M <= 16) return sweep_bn<16>(a, epi, norm, bn, pf, (hipStream_t)stream);
  return sweep_bn<32>(a, epi, norm, bn, pf, (hipStream_t)stream);
}
#endif
