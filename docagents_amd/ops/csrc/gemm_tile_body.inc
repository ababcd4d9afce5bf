// The body of the LDS-staged MFMA tile kernels: gemm_bf16_kernel (gemm.hip, bf16 weights) and
// gemm_tile_w8_kernel (gemm_tile_w8.hip, e4m3 weights with one fp32 scale per weight row). Included
// inside each __global__ kernel, whose template parameters BM, BN, WM, WN, EPI, PF and argument
// `GemmArgs p` it uses, after `constexpr bool W8 = ..., W_NT = ...;` (text, not an inlined function:
// see gemm_dk.h). W8: p.W points at e4m3 codes ([N, K] bytes), streamed 16 codes per load (W_NT:
// non-temporal) and unpacked to bf16 on the way into LDS (cvt16_bf16, exact: one load fills two of the
// 16-B LDS chunks); from LDS on the two kernels are one MFMA sequence, and p.sw[n] multiplies the
// fp32 value of column n first thing in the epilogue (a power-of-two scale commutes with every
// rounding: bit-identical to the bf16 kernel on the dequantised matrix).
  // PF = k-tiles in flight in registers. PF = 1: the classic register-staged double buffer (one
  // tile ahead). Decode-sized tiles (M <= 64) stream weights and are latency-bound at PF = 1 —
  // one 16-KB W tile per workgroup in flight, ~6 dependent HBM round trips per split — so they
  // keep PF tiles (up to 72 KB per workgroup) requested ahead of the MFMAs (Little's law).
  // (Weight fragments loaded straight into the MFMA B registers, skipping LDS, lost on every arm
  // measured: half-line requests, profiles/r3/rejected_r3.txt.)
  constexpr int BK = 64;
  constexpr int TM = BM / WM, TN = BN / WN;
  constexpr int FM = TM / 16, FN = TN / 16;
  constexpr int A_BYTES = BM * BK * 2, B_BYTES = BN * BK * 2;
  constexpr int LA = BM * 8 / 256, LB = BN * 8 / 256;  // 16-B loads per thread per tile
  constexpr int LBR = W8 ? LB / 2 : LB;                // W8: 16 codes per load, two LDS chunks
  static_assert(!W8 || (LB % 2 == 0 && EPI != EPI_GELU && EPI != EPI_ROPE), "fp8 weights: tile / epilogue");
  static_assert(WM * WN == 4, "4 waves");
  static_assert(LA >= 1 && LB >= 1, "tile too small");
  constexpr int STAGE_FLOATS = 4 * TM * (TN + 4);
  constexpr int LDS_MAIN = 2 * (A_BYTES + B_BYTES);
  constexpr int LDS_BYTES = LDS_MAIN > STAGE_FLOATS * 4 ? LDS_MAIN : STAGE_FLOATS * 4;
  __shared__ __attribute__((aligned(16))) char smem[LDS_BYTES];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;

  // ---- tile scheduling: XCD remap, then grouped-M ordering ----
  const int ntm = (p.M + BM - 1) / BM, ntn = (p.N + BN - 1) / BN;
  const int nwg = ntm * ntn;
  const int t = xcd_remap(blockIdx.x, nwg);
  constexpr int GROUP = 8;
  const int gid = t / (GROUP * ntn);
  const int first_m = gid * GROUP;
  const int gsz = min(ntm - first_m, GROUP);
  const int tin = t % (GROUP * ntn);
  const int tm = first_m + tin % gsz, tn = tin / gsz;
  const int m0 = tm * BM, n0 = tn * BN;

  const int kbeg = blockIdx.z * p.k_per_split;
  const int nk = p.k_per_split / BK;

  // ---- global -> register staging (PF slots) ----
  u32x4_t ra[PF][LA], rb[PF][LBR];
  const int fr = lane & 15, fg = lane >> 4;
  // Rows past M / N are clamped, not branched around: they only feed accumulators whose outputs
  // are never stored, and branch-free loads keep the compiler's vmcnt waits counted (a load
  // under a divergent branch makes every later wait a full vmcnt(0) drain).
  auto gload = [&](u32x4_t (&xa)[LA], u32x4_t (&xb)[LBR], int kt) {
    const int k0 = kbeg + kt * BK;
#pragma unroll
    for (int i = 0; i < LA; ++i) {
      const int idx = tid + 256 * i, r = idx >> 3, c = idx & 7;
      xa[i] = *(const u32x4_t*)(p.A + (size_t)min(m0 + r, p.M - 1) * p.lda + k0 + c * 8);
    }
    if constexpr (W8) {  // 64 codes per row and k-tile: 4 lanes x 16 B
#pragma unroll
      for (int i = 0; i < LBR; ++i) {
        const int idx = tid + 256 * i, r = idx >> 2, c = idx & 3;
        const u32x4_t* src = (const u32x4_t*)((const uint8_t*)p.W + (size_t)min(n0 + r, p.N - 1) * p.K + k0 + c * 16);
        xb[i] = W_NT ? __builtin_nontemporal_load(src) : *src;
      }
    } else {
#pragma unroll
      for (int i = 0; i < LB; ++i) {
        const int idx = tid + 256 * i, r = idx >> 3, c = idx & 7;
        xb[i] = *(const u32x4_t*)(p.W + (size_t)min(n0 + r, p.N - 1) * p.K + k0 + c * 8);
      }
    }
  };
  auto lstore = [&](const u32x4_t (&xa)[LA], const u32x4_t (&xb)[LBR], int buf) {
    char* sa = smem + buf * (A_BYTES + B_BYTES);
    char* sb = sa + A_BYTES;
#pragma unroll
    for (int i = 0; i < LA; ++i) {
      const int idx = tid + 256 * i, r = idx >> 3, c = idx & 7;
      *(u32x4_t*)(sa + r * 128 + ((c ^ ((r >> 1) & 7)) << 4)) = xa[i];
    }
    if constexpr (W8) {
#pragma unroll
      for (int i = 0; i < LBR; ++i) {
        const int idx = tid + 256 * i, r = idx >> 2, c = (idx & 3) * 2;
        u32x4_t lo, hi;
        cvt16_bf16(xb[i], lo, hi);
        *(u32x4_t*)(sb + r * 128 + ((c ^ ((r >> 1) & 7)) << 4)) = lo;
        *(u32x4_t*)(sb + r * 128 + (((c + 1) ^ ((r >> 1) & 7)) << 4)) = hi;
      }
    } else {
#pragma unroll
      for (int i = 0; i < LB; ++i) {
        const int idx = tid + 256 * i, r = idx >> 3, c = idx & 7;
        *(u32x4_t*)(sb + r * 128 + ((c ^ ((r >> 1) & 7)) << 4)) = xb[i];
      }
    }
  };

  f32x4_t acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // Loads are issued unconditionally (tile index clamped to nk - 1: the redundant tail loads hit
  // L2) so every vmcnt wait below stays counted; compute / LDS stores sit under uniform branches.
  const int kl = nk > 0 ? nk - 1 : 0;
#pragma unroll
  for (int u = 0; u < PF; ++u) {
    gload(ra[u], rb[u], min(u, kl));
    asm volatile("" ::: "memory");  // keep issue order = tile order (counted waits stay short)
  }
  if (nk > 0) lstore(ra[0], rb[0], 0);
  __syncthreads();

  for (int kt0 = 0; kt0 < nk; kt0 += PF) {
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      const int kt = kt0 + u;
      const int cur = kt & 1;
      // slot u held tile kt, already copied to LDS: refill it PF tiles ahead
      if (PF > 1 || kt + 1 < nk) gload(ra[u], rb[u], min(kt + PF, kl));
      if (kt < nk) {
        const char* sa = smem + cur * (A_BYTES + B_BYTES);
        const char* sb = sa + A_BYTES;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          const int c = kk * 4 + fg;
          bf16x8_t af[FM], bfr[FN];
#pragma unroll
          for (int i = 0; i < FM; ++i) {
            const int r = wm * TM + i * 16 + fr;
            af[i] = *(const bf16x8_t*)(sa + r * 128 + ((c ^ ((r >> 1) & 7)) << 4));
          }
#pragma unroll
          for (int j = 0; j < FN; ++j) {
            const int r = wn * TN + j * 16 + fr;
            bfr[j] = *(const bf16x8_t*)(sb + r * 128 + ((c ^ ((r >> 1) & 7)) << 4));
          }
#pragma unroll
          for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int j = 0; j < FN; ++j) acc[i][j] = mfma16(af[i], bfr[j], acc[i][j]);
        }
      }
      if (kt >= nk) continue;
      if (kt + 1 < nk) lstore(ra[(u + 1) % PF], rb[(u + 1) % PF], cur ^ 1);
      // LDS writes visible + buffer reads done; a raw barrier, NOT __syncthreads(): its fence
      // drains vmcnt and would cancel the PF - 1 tiles still in flight
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
  }

  // ---- epilogue: stage fp32 tile of this wave in LDS, then coalesced 16-B stores ----
  float* st = (float*)smem + wid * TM * (TN + 4);
  constexpr int SLD = TN + 4;
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) st[(i * 16 + fg * 4 + q) * SLD + j * 16 + fr] = acc[i][j][q];
  __syncthreads();

  const int row0 = m0 + wm * TM, col0 = n0 + wn * TN;
  if constexpr (EPI == EPI_SWIGLU) {
    // output tile TM x TN/2; chunk of 8 outputs; TN/16 chunks per row
    constexpr int CPR = TN / 16;
    constexpr int RPI = 64 / CPR;
    const int oc = (lane % CPR) * 8;          // output col within wave tile
    const int grp = oc / 16, within = oc % 16;  // gate cols 32*grp+within.., up cols +16
    const int ncols_out = p.N / 2;
    const int gout = col0 / 2 + oc;
    for (int rr = lane / CPR; rr < TM; rr += RPI) {
      const int gm = row0 + rr;
      if (gm >= p.M || gout >= ncols_out) continue;
      const float* srow = st + rr * SLD + grp * 32 + within;
      float sc[16];  // W8: the scales of the 8 gate rows and of the 8 up rows
      if constexpr (W8) {
        const float* sg = p.sw + col0 + grp * 32 + within;
#pragma unroll
        for (int e = 0; e < 8; ++e) { sc[e] = sg[e]; sc[8 + e] = sg[16 + e]; }
      }
      unsigned packed[4];
#pragma unroll
      for (int e = 0; e < 8; e += 2) {
        float g0 = srow[e], g1 = srow[e + 1], u0 = srow[16 + e], u1 = srow[16 + e + 1];
        if constexpr (W8) { g0 *= sc[e]; g1 *= sc[e + 1]; u0 *= sc[8 + e]; u1 *= sc[8 + e + 1]; }
        packed[e / 2] = pack_bf2(silu(g0) * u0, silu(g1) * u1);
      }
      *(u32x4_t*)(p.C + (size_t)gm * p.ldc + gout) = u32x4_t{packed[0], packed[1], packed[2], packed[3]};
    }
  } else {
    constexpr int CPR = TN / 8;
    constexpr int RPI = 64 / CPR;
    const int cc = (lane % CPR) * 8;
    const int gn = col0 + cc;
    for (int rr = lane / CPR; rr < TM; rr += RPI) {
      const int gm = row0 + rr;
      if (gm >= p.M || gn >= p.N) continue;
      const float* srow = st + rr * SLD + cc;
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = srow[e];
      if constexpr (W8) {
        const f32x4_t s0 = *(const f32x4_t*)(p.sw + gn), s1 = *(const f32x4_t*)(p.sw + gn + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[e] *= s0[e]; v[4 + e] *= s1[e]; }
      }
      if constexpr (EPI == EPI_PARTIAL) {
        float* dst = p.ws + ((size_t)blockIdx.z * p.M + gm) * p.N + gn;
        *(f32x4_t*)dst = f32x4_t{v[0], v[1], v[2], v[3]};
        *(f32x4_t*)(dst + 4) = f32x4_t{v[4], v[5], v[6], v[7]};
        continue;
      }
      if (p.bias) {
        u32x4_t b = *(const u32x4_t*)(p.bias + gn);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[2 * e] += bf2f((bf16_t)(b[e] & 0xffff));
          v[2 * e + 1] += bf2f((bf16_t)(b[e] >> 16));
        }
      }
      if constexpr (EPI == EPI_GELU) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = gelu_erf(v[e]);
      }
      if constexpr (EPI == EPI_RESID) {
        u32x4_t r = *(const u32x4_t*)(p.resid + (size_t)gm * p.ldr + gn);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[2 * e] += bf2f((bf16_t)(r[e] & 0xffff));
          v[2 * e + 1] += bf2f((bf16_t)(r[e] >> 16));
        }
      }
      *(u32x4_t*)(p.C + (size_t)gm * p.ldc + gn) =
          u32x4_t{pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]), pack_bf2(v[4], v[5]), pack_bf2(v[6], v[7])};
    }
  }
