// The gemm_dk kernel body: C[M, N'] = epi( rownorm(A)[M, K] . W[N, K]^T ), one BM x BN output tile per
// 256-thread workgroup. Included inside a __global__ kernel template <BM, BN, EPI, NORM, PF> whose
// argument is `p` (WS::Args), after `using WS = DkWBf16 / DkWFp8;` (gemm_dk.h). Design notes: gemm_dk.hip.
  constexpr int FM = BM / 16, FN = BN / 16;
  constexpr int KC = 256;                       // k per chunk: one 64-deep k-tile per wave
  constexpr int ROWB = KC * 2;                  // 512 B per staged row
  constexpr int LW = WS::lw(BN), LA = BM / 8;   // 16-B pieces per thread per chunk (A: 32 per row)
  constexpr int CHUNK = (BN + BM) * ROWB;
  constexpr int SLD = BN + 4;
  constexpr int RED = 4 * BM * SLD * 4;
  constexpr int LDS_BYTES = 2 * CHUNK > RED ? 2 * CHUNK : RED;
  __shared__ __attribute__((aligned(16))) char smem[LDS_BYTES];
  __shared__ float sinv[BM];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  // row blocks (M > BM): rb = 2, and the two row blocks of an n-tile are workgroups i and i + 8 —
  // the same XCD under round-robin placement, dispatched together, so the second reads W from L2
  int tile = blockIdx.x, m0 = 0;
  if constexpr (WS::kRowBlocks) {
    if (p.rb == 2) {
      const int g = blockIdx.x >> 4, wi = blockIdx.x & 15;
      tile = g * 8 + (wi & 7);
      m0 = (wi >> 3) * BM;
    }
  }
  if (tile * BN >= p.N || (WS::kRowBlocks && m0 >= p.M)) return;  // whole-workgroup exit (grid padded to 16)
  const int n0 = tile * BN;
  const int Mb = min(BM, p.M - m0);  // rows of this block
  const int nch = p.K / KC;
  const int kl = nch - 1;

  // ---- global -> registers: whole row segments, W non-temporal (streamed once), A through the caches ----
  u32x4_t rw[PF][LW], ra[PF][LA];
  auto gload = [&](u32x4_t (&xw)[LW], u32x4_t (&xa)[LA], int c) {
    const int k0 = c * KC;
#pragma unroll
    for (int i = 0; i < LW; ++i) xw[i] = WS::load(p, i, tid, n0, k0);
#pragma unroll
    for (int i = 0; i < LA; ++i) {
      const int idx = tid + 256 * i, r = idx >> 5, ch = idx & 31;
      xa[i] = *(const u32x4_t*)(p.A + (size_t)(m0 + min(r, Mb - 1)) * p.lda + k0 + ch * 8);
    }
  };
  auto lstore = [&](const u32x4_t (&xw)[LW], const u32x4_t (&xa)[LA], int buf) {
    char* sw = smem + buf * CHUNK;
    char* sa = sw + BN * ROWB;
#pragma unroll
    for (int i = 0; i < LW; ++i) WS::store(sw, i, tid, xw[i]);
#pragma unroll
    for (int i = 0; i < LA; ++i) {
      const int idx = tid + 256 * i, r = idx >> 5, ch = idx & 31;
      *(u32x4_t*)dk_slot(sa, r, ch) = xa[i];
    }
  };

#pragma unroll
  for (int u = 0; u < PF; ++u) {
    gload(rw[u], ra[u], min(u, kl));
    asm volatile("" ::: "memory");  // issue order = chunk order (counted waits)
  }
  // ---- deferred RMSNorm: inv[m] from the producer's per-part sums (fixed summation order) ----
  if constexpr (NORM) {
    // thread = (part lane, 4-row quad): a few independent 16-B loads per thread (a per-row serial
    // walk over the ~200 parts was ~25 dependent L2 round trips), partials combined in LDS in a
    // fixed order
    constexpr int RQ = BM / 4, PL = 256 / RQ;
    __shared__ f32x4_t sq4[PL][RQ];
    const int rq = tid % RQ, pl = tid / RQ;
    f32x4_t a4{0.f, 0.f, 0.f, 0.f};
    // 8 parts' loads issued before their adds (clamped; + 0 past the end is exact: sums of squares
    // are never -0): with ~192 parts on 64 part lanes, `#pragma unroll 4` left a 3-trip remainder
    // loop that waited for each load in turn
    for (int q0 = pl; q0 < p.ssq_parts; q0 += 8 * PL) {
      f32x4_t v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        v[j] = *(const f32x4_t*)(p.ssq_in + (size_t)min(q0 + j * PL, p.ssq_parts - 1) * 64 + m0 + 4 * rq);
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
  for (int t = tid; t < BM * CPR; t += 256) {
    const int m = t / CPR, ch = t % CPR;
    float v[8];
    if constexpr (EPI == EPI_SWIGLU) {
      const int g = ch >> 1, hh = ch & 1;
      const int gc = 32 * g + 8 * hh;
      float sg[8], su[8];
      WS::scales8(p, n0 + gc, sg);
      WS::scales8(p, n0 + gc + 16, su);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float gt = red[0][m][gc + e] + red[1][m][gc + e] + red[2][m][gc + e] + red[3][m][gc + e];
        const float up = red[0][m][gc + 16 + e] + red[1][m][gc + 16 + e] + red[2][m][gc + 16 + e] +
                         red[3][m][gc + 16 + e];
        if constexpr (WS::kScaled) v[e] = silu(gt * sg[e]) * (up * su[e]);
        else v[e] = silu(gt) * up;
      }
      const int oc = n0 / 2 + 16 * g + 8 * hh;
      if (m < Mb && oc < p.N / 2) {  // a ragged last tile (N % BN == 32) holds one gate/up group
        *(u32x4_t*)(p.C + (size_t)(m0 + m) * p.ldc + oc) =
            u32x4_t{pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]), pack_bf2(v[4], v[5]), pack_bf2(v[6], v[7])};
      }
    } else {
      const int c = 8 * ch;
      const int gn = n0 + c;
      const bool ok = m < Mb && gn < p.N;
      float sc[8];
      WS::scales8(p, gn, sc);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        v[e] = red[0][m][c + e] + red[1][m][c + e] + red[2][m][c + e] + red[3][m][c + e];
        if constexpr (WS::kScaled) v[e] *= sc[e];
      }
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
          const u32x4_t r = *(const u32x4_t*)(p.resid + (size_t)(m0 + m) * p.ldr + gn);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            v[2 * e] += bf2f((bf16_t)(r[e] & 0xffff));
            v[2 * e + 1] += bf2f((bf16_t)(r[e] >> 16));
          }
        }
      }
      const u32x4_t o{pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]), pack_bf2(v[4], v[5]), pack_bf2(v[6], v[7])};
      if (ok) *(u32x4_t*)(p.C + (size_t)(m0 + m) * p.ldc + gn) = o;
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
          if (ch == 0) p.ssq_out[(size_t)tile * 64 + m0 + m] = sq;
        }
      }
    }
  }
