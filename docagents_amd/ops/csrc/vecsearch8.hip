// fp8 (OCP e4m3) vector index rows (INDEX_DTYPE=fp8, INDEX_KIND=ivfflat_fp8): the row quantiser (in
// place and scattered), the row dequantiser and the k-means update over codes that IVFFlat training
// uses, and the fp8 forms of the index scans of vecsearch.hip.
//
// Storage: a row of d values is d e4m3 codes plus ONE fp32 power-of-two scale: the smallest 2^e with
// amax / 2^e <= 448 (1 for an all-zero row): fp8_pow2_scale (fp8.h). code * 2^e is exact in bf16.
//   codes [N, d]  one byte each        scale [N] fp32
// A scan streams d + 4 bytes per row instead of 2 d. Queries stay bf16 and the MFMA stays bf16: the
// codes are unpacked in registers (cvt8_bf16, fp8.h — exact), so a score is
// scale[row] * sum(code_i * q_i) with fp32 accumulation: the search of the bf16 matrix codes * scale,
// up to fp32 summation order. Candidate lists (TdWave) and the final merge are the bf16 scans'.
#include "fp8.h"
#include "vecsearch_topk.h"

extern "C" int da_topk_merge(void* cand_s, void* cand_i, int P, int Q, int K, void* out_s, void* out_i, void* stream);

// ------------------------------------------------------------------------------------------------
// One bf16 row xr[d] -> its codes cr[d] and its scale *sp, by one wave (4 elements per lane per step
// of 256): amax over the row by lane shuffles, then fp8_pow2_scale.
__device__ __forceinline__ void quant_row(const bf16_t* __restrict__ xr, int d, uint8_t* __restrict__ cr,
                                          float* __restrict__ sp, int lane) {
  float amax = 0.f;
  for (int j = lane * 4; j < d; j += 256) {
    const u32x2_t a = *(const u32x2_t*)(xr + j);
    amax = fmaxf(fmaxf(amax, fmaxf(fabsf(bf2f(a[0] & 0xffff)), fabsf(bf2f(a[0] >> 16)))),
                 fmaxf(fabsf(bf2f(a[1] & 0xffff)), fabsf(bf2f(a[1] >> 16))));
  }
  amax = wave_max(amax);
  float sc, inv;
  fp8_pow2_scale(amax, sc, inv);
  for (int j = lane * 4; j < d; j += 256) {
    const u32x2_t a = *(const u32x2_t*)(xr + j);
    *(unsigned*)(cr + j) = f32x4_fp8(bf2f(a[0] & 0xffff), bf2f(a[0] >> 16), bf2f(a[1] & 0xffff), bf2f(a[1] >> 16), inv);
  }
  if (lane == 0) *sp = sc;
}

// bf16 rows X [n, d] -> codes[(row0 + r) * d ..] and scale[row0 + r]. One wave per row. Writes nothing
// outside rows [row0, row0 + n).
__global__ void __launch_bounds__(256)
index_quant_rows_kernel(const bf16_t* __restrict__ X, int n, int d, uint8_t* __restrict__ codes,
                        float* __restrict__ scale, long long row0) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;  // wave-uniform
  quant_row(X + (size_t)r * d, d, codes + ((size_t)row0 + r) * d, scale + row0 + r, lane);
}

// The scatter form (the IVF streaming build): row r of X -> codes[dest[r]], scale[dest[r]], the rows of
// dest distinct. A destination outside [0, cap) is skipped (the wrapper refuses it before the launch).
__global__ void __launch_bounds__(256)
index_quant_scatter_kernel(const bf16_t* __restrict__ X, int n, int d, uint8_t* __restrict__ codes,
                           float* __restrict__ scale, const long long* __restrict__ dest, long long cap) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;  // wave-uniform
  const long long t = dest[r];
  DA_ASSERT(t >= 0 && t < cap);
  if (t < 0 || t >= cap) return;  // wave-uniform
  quant_row(X + (size_t)r * d, d, codes + (size_t)t * d, scale + t, lane);
}

DA_EXPORT int da_index_quant_rows(const void* X, int n, int d, void* codes, void* scale, long long row0,
                                  void* stream) {
  if (d % 4 || d < 4 || n < 0 || row0 < 0 || !X || !codes || !scale) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  index_quant_rows_kernel<<<(n + 3) / 4, 256, 0, (hipStream_t)stream>>>((const bf16_t*)X, n, d, (uint8_t*)codes,
                                                                        (float*)scale, row0);
  DA_LAUNCH_CHECK();
}

DA_EXPORT int da_index_quant_scatter(const void* X, int n, int d, void* codes, void* scale, const void* dest,
                                     long long cap, void* stream) {
  if (d % 4 || d < 4 || n < 0 || cap < 0 || !X || !codes || !scale || !dest) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  index_quant_scatter_kernel<<<(n + 3) / 4, 256, 0, (hipStream_t)stream>>>(
      (const bf16_t*)X, n, d, (uint8_t*)codes, (float*)scale, (const long long*)dest, cap);
  DA_LAUNCH_CHECK();
}

// ------------------------------------------------------------------------------------------------
// codes * scale -> bf16 (exact: fp8.h) for the IVF training paths: out[r] = row row0 + r of the store,
// or row sel[r]. One wave per row, a 16-B piece of codes per lane per step of 1024 -> two 16-B stores.
// d % 16 == 0. A source row outside [0, cap) is skipped (the wrapper refuses it before the launch).
__global__ void __launch_bounds__(256)
index_dequant_rows_kernel(const uint8_t* __restrict__ codes, const float* __restrict__ scale, long long cap, int d,
                          long long row0, const long long* __restrict__ sel, int n, bf16_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;  // wave-uniform
  const long long t = sel ? sel[r] : row0 + r;
  DA_ASSERT(t >= 0 && t < cap);
  if (t < 0 || t >= cap) return;  // wave-uniform
  const float sc = scale[t];
  const uint8_t* cr = codes + (size_t)t * d;
  bf16_t* orow = out + (size_t)r * d;
  for (int j = lane * 16; j < d; j += 1024) {
    const u32x4_t w = *(const u32x4_t*)(cr + j);
    u32x4_t lo, hi;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const f32x4_t f = fp8x4_f32(w[e]);
      const unsigned p0 = pack_bf2(f[0] * sc, f[1] * sc), p1 = pack_bf2(f[2] * sc, f[3] * sc);
      if (e < 2) { lo[2 * e] = p0; lo[2 * e + 1] = p1; } else { hi[2 * e - 4] = p0; hi[2 * e - 3] = p1; }
    }
    *(u32x4_t*)(orow + j) = lo;
    *(u32x4_t*)(orow + j + 8) = hi;
  }
}

DA_EXPORT int da_index_dequant_rows(const void* codes, const void* scale, long long cap, int d, long long row0,
                                    const void* sel, int n, void* out, void* stream) {
  if (d % 16 || d < 16 || n < 0 || cap < 0 || row0 < 0 || !codes || !scale || !out || ((uintptr_t)codes & 15) ||
      ((uintptr_t)out & 15) || (!sel && row0 + n > cap))
    return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  index_dequant_rows_kernel<<<(n + 3) / 4, 256, 0, (hipStream_t)stream>>>(
      (const uint8_t*)codes, (const float*)scale, cap, d, row0, (const long long*)sel, n, (bf16_t*)out);
  DA_LAUNCH_CHECK();
}

// ------------------------------------------------------------------------------------------------
// k-means update over fp8 rows (IVFFlat training on the codes): for every row with assign >= 0,
// sums[assign] += scale[row] * code per element (exact in fp32: an e4m3 value times a power of two)
// and counts[assign] += 1. One wave per row, 4 rows per workgroup. The row is read 16 B per lane
// (1024 codes per step) and turned through LDS so that each atomic wave-instruction adds 64
// neighbouring floats (256 contiguous bytes, the shape float atomics run fastest in); a lane takes the
// dword of its code from LDS and converts the one byte. Rows with assign < 0 and lists that get no
// row add nothing. d % 16 == 0.
__global__ void __launch_bounds__(256)
kmeans_accum8_kernel(const uint8_t* __restrict__ codes, const float* __restrict__ scale, int N, int d,
                     const int* __restrict__ assign, int L, float* __restrict__ sums, float* __restrict__ counts) {
  __shared__ u32x4_t sW[4][64];  // per wave: 1024 codes of its row
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int r = blockIdx.x * 4 + wid;
  int c = -1;
  if (r < N) c = assign[r];
  DA_ASSERT(c < L);
  const bool on = c >= 0 && c < L;  // wave-uniform; every wave keeps the workgroup's barriers
  const float sc = on ? scale[r] : 0.f;
  const uint8_t* cr = codes + (size_t)(on ? r : 0) * d;
  float* srow = sums + (size_t)(on ? c : 0) * d;
  const unsigned* sD = (const unsigned*)sW[wid];
  for (int base = 0; base < d; base += 1024) {
    const int j = base + lane * 16;
    u32x4_t w = u32x4_t{0, 0, 0, 0};
    if (on && j < d) w = *(const u32x4_t*)(cr + j);
    __syncthreads();  // the previous step's reads
    sW[wid][lane] = w;
    __syncthreads();
    if (on) {
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const int e = base + t * 64 + lane;
        if (e < d) {
          const unsigned dw = sD[t * 16 + (lane >> 2)] >> ((lane & 3) * 8);
          atomicAdd(&srow[e], __builtin_amdgcn_cvt_pk_f32_fp8(dw, false)[0] * sc);
        }
      }
    }
  }
  if (on && lane == 0) atomicAdd(&counts[c], 1.f);
}

DA_EXPORT int da_kmeans_accum8(const void* codes, const void* scale, int N, int d, const void* assign, int L,
                               void* sums, void* counts, void* stream) {
  if (d % 16 || d < 16 || N < 0 || L < 1 || !codes || !scale || !assign || !sums || !counts ||
      ((uintptr_t)codes & 15))
    return (int)hipErrorInvalidValue;
  if (N == 0) return 0;
  kmeans_accum8_kernel<<<(N + 3) / 4, 256, 0, (hipStream_t)stream>>>(
      (const uint8_t*)codes, (const float*)scale, N, d, (const int*)assign, L, (float*)sums, (float*)counts);
  DA_LAUNCH_CHECK();
}

// ------------------------------------------------------------------------------------------------
// Streaming dense scan over fp8 rows (d % 64 == 0 here; instantiated for d = 128, 384, 768, 1024):
// the structure of topk_dense_stream_kernel. Every wave is an independent worker over its own run
// of 16-row tiles against the workgroup's <= 16 queries.
//  * Lane (fr, fg) loads, per tile, NL = d / 64 non-temporal 16-B pieces of row fr: bytes
//    64 j + 16 fg .. + 15 (j < NL). A piece carries 16 codes = two k-steps of the 16x16x32 bf16 MFMA:
//    k-step 2 j + h (h = 0, 1) multiplies codes 64 j + 16 fg + 8 h .. + 7 of the row. The query
//    fragment of that k-step holds the same columns (any K permutation shared by both operands is a
//    dot product): the LDS copy of the queries is stored in that order, 16-B chunk 8 j + 2 fg + h of
//    a query row at chunk 4 (2 j + h) + fg, so the read addresses are the bf16 kernel's.
//  * The ring runs TWO tiles ahead (2 * 16 * d bytes per wave in flight, what the bf16 scan keeps
//    with one tile), every load unconditional with clamped rows, so the vmcnt waits stay counted.
//    A tile's four row scales (one aligned 16-B load per lane, rows 4 fg .. + 3 of the tile, the
//    index clamped to the last quad of the shard) are requested just BEFORE the tile's codes, so
//    waiting for the codes has waited for them.
//  * The scale multiplies the finished accumulator before TdWave::tile, so the floor, the running
//    k-th best and the stored score all see final scores.
// scale must be readable up to the next multiple of 4 rows past N (the wrapper guarantees it).
template <int NL>
__global__ void __launch_bounds__(256)
topk_dense_stream8_kernel(const uint8_t* __restrict__ C, const float* __restrict__ scale, int N,
                          const int* __restrict__ slots, const bf16_t* __restrict__ Qv, int Q,
                          const unsigned* __restrict__ bitmap, int W, float thr, int K, int rows_per_wave, int nqb,
                          float* __restrict__ out_s, int* __restrict__ out_i) {
  constexpr int d = NL * 64;
  constexpr int qstr = d * 2 + 16;
  __shared__ __attribute__((aligned(16))) char sQ[16 * qstr];   // [16][d] bf16 (k-permuted), rows padded by 16 B
  __shared__ float cs_all[4][16 * TD_SL];  // per wave: top-K lists + candidate buffers (TdWave)
  __shared__ int ci_all[4][16 * TD_SL];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  // XCD-grouped block order, as topk_dense_stream_kernel
  const int b = blockIdx.x, per = 8 * nqb;
  const int grp = b / per, rem = b % per;
  const int qb = rem / 8, rb = grp * 8 + rem % 8;
  const int qbase = qb * 16, nq = min(16, Q - qbase);
  for (int i = tid; i < 16 * (d / 8); i += 256) {
    const int r = i / (d / 8), c = i % (d / 8);
    u32x4_t v = u32x4_t{0, 0, 0, 0};
    if (r < nq) v = *(const u32x4_t*)(Qv + (size_t)(qbase + r) * d + c * 8);
    const int dc = (((c >> 3) * 2 + (c & 1)) << 2) + ((c >> 1) & 3);
    *(u32x4_t*)(sQ + r * qstr + dc * 16) = v;
  }
  TdWave st;
  st.init(cs_all[wid], ci_all[wid], K);
  __syncthreads();

  const int wbeg = (int)min((long)N, ((long)rb * 4 + wid) * rows_per_wave);
  const int wend = (int)min((long)N, (long)wbeg + rows_per_wave);
  DA_ASSERT(wbeg == N || wbeg % 16 == 0);
  const int ntile = (wend - wbeg + 15) / 16;
  const int lrow = N - 1, lquad = (N - 1) & ~3;
  auto sload = [&](int t) {  // the scales of rows 4 fg .. + 3 of tile t (clamped)
    return *(const f32x4_t*)(scale + min(wbeg + t * 16 + fg * 4, lquad));
  };
  auto rowp = [&](int t) {  // this lane's first piece of tile t (row clamped)
    return C + (size_t)min(wbeg + t * 16 + fr, lrow) * d + fg * 16;
  };
  u32x4_t ring[2][NL];
  f32x4_t scr[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    scr[u] = sload(u);
    const uint8_t* p = rowp(u);
#pragma unroll
    for (int j = 0; j < NL; ++j) ring[u][j] = __builtin_nontemporal_load((const u32x4_t*)(p + j * 64));
    asm volatile("" ::: "memory");  // issue order = tile order (counted waits)
  }
  const bool qok = fr < nq;
  // whole pairs of tiles (the ring keeps fixed registers); a tile past the end re-reads clamped rows
  // and every row of it is masked
  for (int t0 = 0; t0 < ntile; t0 += 2) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int t = t0 + u;
      f32x4_t acc = f32x4_t{0.f, 0.f, 0.f, 0.f};
      const f32x4_t sc = scr[u];
      scr[u] = sload(t + 2);
      const uint8_t* pn = rowp(t + 2);
#pragma unroll
      for (int j = 0; j < NL; ++j) {
        const u32x4_t w = ring[u][j];
        const bf16x8_t b0 = *(const bf16x8_t*)(sQ + fr * qstr + (2 * j) * 64 + fg * 16);
        const bf16x8_t b1 = *(const bf16x8_t*)(sQ + fr * qstr + (2 * j + 1) * 64 + fg * 16);
        acc = mfma16(cvt8_bf16(w[0], w[1]), b0, acc);
        acc = mfma16(cvt8_bf16(w[2], w[3]), b1, acc);
        // piece j of tile t + 2 into the slot just consumed
        ring[u][j] = __builtin_nontemporal_load((const u32x4_t*)(pn + j * 64));
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] *= sc[i];
      st.tile(acc, wbeg + t * 16 + fg * 4, wend, qok, thr, slots, bitmap, W, qbase + fr);
    }
  }
  st.finish();
  // the 4 waves' lists -> one per workgroup (wave 0 absorbs the others'), out [rb, Q, K]
  __syncthreads();
  if (wid == 0) {
    for (int w = 1; w < 4; ++w) st.absorb(cs_all[w], ci_all[w], nq);
    st.store(nq, ((size_t)rb * Q + qbase) * K, out_s, out_i);
  }
}

// 17+ queries: the fp8 form of topk_dense_mq_kernel. The workgroup's 4 waves = 4 query blocks over
// the SAME rows; a tile is read from HBM once into LDS and feeds all four waves, whose B fragments
// (k-permuted as above) live in registers. An LDS tile is 32 rows x d bytes — the bytes of the bf16
// kernel's 16-row tile, so NG = d / 128 16-B loads per thread again — and holds two 16-row MFMA
// tiles; TD8_PF LDS tiles in flight in registers (with their scales, requested before the codes), two
// LDS buffers, one barrier per LDS tile. rows_per_block % 32 == 0.
// LDS image: a row is CPR = d / 16 chunks of 16 B, rows back to back, so row r starts at slot
// (r * CPR) % 16 of the 256-B bank row: 0 for every row when CPR % 16 == 0 (d = 768, 1024), and
// 8 (r & 1) when CPR % 16 == 8 (d = 128, 384). A ds_read_b128 lane group is 16 lanes with 16
// distinct fr, 8 of them with fg = f and 8 with fg = f ^ 1 ({0-3, 12-15} and {4-11}), reading chunk
// 4 s + fg of row fr. Chunk c of row r is stored at c ^ x(r):
//   CPR % 16 == 0: x = r & 15      — the bf16 kernel's swizzle: 16 rows -> 16 slots
//   CPR % 16 == 8: x = (r >> 1) & 7 — stays inside the row's aligned 8 chunks; slot = 8 ((r & 1) ^
//                  (c >> 3 & 1)) + ((c & 7) ^ x): rows 2 x, 2 x + 1 take the two halves of the bank
//                  row, and the group's two fg sets map to disjoint x ^ (c & 7) sets
// both conflict-free for the read above. (r & 15 on a 128-B row would leave the row.)
constexpr int TD8_PF = 3;

template <int NG>
__global__ void __launch_bounds__(256, 1)
topk_dense_mq8_kernel(const uint8_t* __restrict__ C, const float* __restrict__ scale, int N,
                      const int* __restrict__ slots, const bf16_t* __restrict__ Qv, int Q,
                      const unsigned* __restrict__ bitmap, int W, float thr, int K, int rows_per_block, int nqg,
                      float* __restrict__ out_s, int* __restrict__ out_i) {
  constexpr int d = NG * 128, NS = d / 64, CPR = d / 16, TB = 32 * d;
  constexpr int XS = (CPR % 16) ? 1 : 0, XM = (CPR % 16) ? 7 : 15;
  static_assert(32 * CPR == 256 * NG, "one 16-B load per thread per 128 columns");
  static_assert(CPR % 8 == 0, "the swizzle stays inside aligned runs of 8 chunks");
  __shared__ __attribute__((aligned(16))) char sX[2][TB];
  __shared__ float cs_all[4][16 * TD_SL];
  __shared__ int ci_all[4][16 * TD_SL];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const int b = blockIdx.x, per = 8 * nqg;
  const int grp = b / per, rem = b % per;
  const int qg = rem / 8, rb = grp * 8 + rem % 8;
  const int qbase = (qg * 4 + wid) * 16, nq = max(0, min(16, Q - qbase));
  const bool qok = fr < nq;
  // this wave's B fragments: query qbase + fr, k-step 2 s + h = columns 64 s + 16 fg + 8 h .. + 7
  bf16x8_t bq[2 * NS];
#pragma unroll
  for (int kk = 0; kk < 2 * NS; ++kk)
    bq[kk] = qok ? *(const bf16x8_t*)(Qv + (size_t)(qbase + fr) * d + (kk >> 1) * 64 + fg * 16 + (kk & 1) * 8)
                 : bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0};
  TdWave st;
  st.init(cs_all[wid], ci_all[wid], K);

  const int rbeg = (int)min((long)N, (long)rb * rows_per_block);
  const int rend = (int)min((long)N, (long)rbeg + rows_per_block);
  DA_ASSERT(rows_per_block % 32 == 0);
  const int ntile = (rend - rbeg + 31) / 32;
  const int tl = max(ntile - 1, 0), lrow = N - 1, lquad = (N - 1) & ~3;
  // LDS tile t (rows clamped): the scales of this lane's rows in both MFMA tiles, then the thread's
  // chunks tid + 256 i
  auto gload = [&](u32x4_t (&v)[NG], f32x4_t (&sc)[2], int t) {
#pragma unroll
    for (int m = 0; m < 2; ++m) sc[m] = *(const f32x4_t*)(scale + min(rbeg + t * 32 + m * 16 + fg * 4, lquad));
#pragma unroll
    for (int i = 0; i < NG; ++i) {
      const int idx = tid + 256 * i, r = idx / CPR, c = idx % CPR;
      v[i] = __builtin_nontemporal_load((const u32x4_t*)(C + (size_t)min(rbeg + t * 32 + r, lrow) * d + c * 16));
    }
  };
  auto lstore = [&](const u32x4_t (&v)[NG], int buf) {
#pragma unroll
    for (int i = 0; i < NG; ++i) {
      const int idx = tid + 256 * i, r = idx / CPR, c = idx % CPR;
      *(u32x4_t*)(&sX[buf][r * d + ((c ^ ((r >> XS) & XM)) << 4)]) = v[i];
    }
  };
  __syncthreads();  // the lists' initial values (before any load is in flight: this drains them)
  u32x4_t ring[TD8_PF][NG];
  f32x4_t scr[TD8_PF][2];
#pragma unroll
  for (int u = 0; u < TD8_PF; ++u) {
    gload(ring[u], scr[u], min(u, tl));
    asm volatile("" ::: "memory");  // issue order = tile order (counted waits)
  }
  const int xr = (fr >> XS) & XM;
  // whole groups of TD8_PF tiles (no exit inside the unrolled group: the ring keeps fixed registers);
  // tiles past the end re-read the last one and mask every row
  for (int t0 = 0; t0 < ntile; t0 += TD8_PF) {
#pragma unroll
    for (int u = 0; u < TD8_PF; ++u) {
      const int t = t0 + u;
      const int buf = t & 1;
      lstore(ring[u], buf);
      const f32x4_t sc0 = scr[u][0], sc1 = scr[u][1];
      gload(ring[u], scr[u], min(t + TD8_PF, tl));  // clamped past the end: uniform counts
      // tile t visible to every wave, and every wave is done with tile t - 2 (same buffer): a raw
      // barrier (__syncthreads() would drain the loads in flight)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      f32x4_t acc0 = f32x4_t{0.f, 0.f, 0.f, 0.f}, acc1 = f32x4_t{0.f, 0.f, 0.f, 0.f};
      const char* x0 = &sX[buf][fr * d];
      const char* x1 = &sX[buf][(16 + fr) * d];
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const int c = ((s * 4 + fg) ^ xr) << 4;
        const u32x4_t w0 = *(const u32x4_t*)(x0 + c);
        const u32x4_t w1 = *(const u32x4_t*)(x1 + c);
        acc0 = mfma16(cvt8_bf16(w0[0], w0[1]), bq[2 * s], acc0);
        acc1 = mfma16(cvt8_bf16(w1[0], w1[1]), bq[2 * s], acc1);
        acc0 = mfma16(cvt8_bf16(w0[2], w0[3]), bq[2 * s + 1], acc0);
        acc1 = mfma16(cvt8_bf16(w1[2], w1[3]), bq[2 * s + 1], acc1);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) { acc0[i] *= sc0[i]; acc1[i] *= sc1[i]; }
      st.tile(acc0, rbeg + t * 32 + fg * 4, rend, qok, thr, slots, bitmap, W, qbase + fr);
      st.tile(acc1, rbeg + t * 32 + 16 + fg * 4, rend, qok, thr, slots, bitmap, W, qbase + fr);
    }
  }
  st.finish();
  st.store(nq, ((size_t)rb * Q + qbase) * K, out_s, out_i);
}

// Per-query row ranges over fp8 rows: topk_ranges_kernel with 16 codes per lane per load, an fp32 FMA
// chain, and the row's scale applied after the half-wave reduction. d % 16 == 0, d <= 4096.
__global__ void __launch_bounds__(256)
topk_ranges8_kernel(const uint8_t* __restrict__ C, const float* __restrict__ scale, int d,
                    const int* __restrict__ slots, const bf16_t* __restrict__ Qv, int Q,
                    const int* __restrict__ ranges, const int* __restrict__ range_off,
                    const unsigned* __restrict__ bitmap, int W, float thr, int K, int rows_per_split,
                    float* __restrict__ out_s, int* __restrict__ out_i) {
  __shared__ float sc[64];
  __shared__ int sr[64];
  __shared__ float best[TK_MAX];
  __shared__ int bidx[TK_MAX];
  const int split = blockIdx.x, q = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int half = lane >> 5, l32 = lane & 31;
  if (tid < TK_MAX) { best[tid] = -INFINITY; bidx[tid] = -1; }
  // query chunks (16 columns) held in registers: lane handles chunks c = l32 + 32*i
  constexpr int MAXC = 8;  // d <= 32 * 16 * 8 = 4096
  const int nch = d / 16;
  float qv[MAXC][16];
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int c = l32 + 32 * i;
    if (c < nch) {
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        u32x4_t u = *(const u32x4_t*)(Qv + (size_t)q * d + c * 16 + hh * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e)
          qv[i][hh * 8 + e] = bf2f((bf16_t)((e & 1) ? (u[e >> 1] >> 16) : (u[e >> 1] & 0xffff)));
      }
    }
  }
  const int rb = range_off[q], re = range_off[q + 1];
  DA_ASSERT(rb >= 0 && re >= rb);
  const int pbeg = split * rows_per_split, pend = pbeg + rows_per_split;
  __syncthreads();
  // walk the concatenated ranges; position p counts rows across this query's ranges
  int pos = 0;
  for (int r = rb; r < re; ++r) {
    const int s0 = ranges[2 * r], s1 = ranges[2 * r + 1];
    DA_ASSERT(s0 >= 0 && s1 >= s0);
    const int len = s1 - s0;
    const int lo = max(pbeg, pos), hi = min(pend, pos + len);
    for (int p0 = lo; p0 < hi; p0 += 64) {
      // 64 rows per iteration: 8 half-waves x 8 rows
      for (int j = 0; j < 8; ++j) {
        const int rl = (wid * 2 + half) * 8 + j;
        const int p = p0 + rl;
        float dot = 0.f;
        const int row = s0 + (p - pos);
        if (p < hi) {
          const uint8_t* cr = C + (size_t)row * d;
#pragma unroll
          for (int i = 0; i < MAXC; ++i) {
            const int c = l32 + 32 * i;
            if (c < nch) {
              const u32x4_t u = *(const u32x4_t*)(cr + c * 16);
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const f32x4_t f = fp8x4_f32(u[e]);
#pragma unroll
                for (int x = 0; x < 4; ++x) dot += qv[i][4 * e + x] * f[x];
              }
            }
          }
        }
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
        if (l32 == 0) {
          if (p < hi) dot *= scale[row];
          bool ok = p < hi && dot >= thr;
          if (ok && slots) {
            const int sl = slots[row];
            ok = sl >= 0 && (!bitmap || ((sl >> 5) < W && ((bitmap[(size_t)q * W + (sl >> 5)] >> (sl & 31)) & 1u)));
          }
          sc[rl] = ok ? dot : -INFINITY;
          sr[rl] = ok ? row : -1;
        }
      }
      __syncthreads();
      if (wid == 0) wave_merge_topk(sc[lane], sr[lane], best, bidx, K, lane);
      __syncthreads();
    }
    pos += len;
    if (pos >= pend) break;
  }
  if (tid < K) {
    const size_t o = ((size_t)split * Q + q) * K + tid;
    out_s[o] = best[tid];
    out_i[o] = bidx[tid];
  }
}

// ws of da_topk_dense_stream8: (row blocks padded to 8) * Q * K candidate pairs
DA_EXPORT size_t da_topk_dense_stream8_ws(int N, int Q, int K, int rows_per_wave) {
  const long nrb = ((long)N + 4L * rows_per_wave - 1) / (4L * rows_per_wave);
  const long nrb8 = (nrb + 7) / 8 * 8;
  return (size_t)nrb8 * Q * K * 8;
}

// The fp8 dense scan (d = 128, 384, 768 or 1024; rows_per_wave % 16 == 0; codes 16-B aligned, scale
// 16-B aligned and readable up to the next multiple of 4 rows). hipErrorInvalidValue for shapes it
// does not take: there is no other fp8 dense kernel behind it.
DA_EXPORT int da_topk_dense_stream8(const void* codes, const void* scale, int N, int d, const void* slots,
                                    const void* Qv, int Q, const void* bitmap, int W, float thr, int K,
                                    int rows_per_wave, void* ws, void* out_s, void* out_i, void* stream) {
  if ((d != 128 && d != 384 && d != 768 && d != 1024) || K < 1 || K > TK_MAX || rows_per_wave % 16 ||
      rows_per_wave <= 0 || N < 1 || !codes || !scale || ((uintptr_t)codes & 15) || ((uintptr_t)scale & 15))
    return (int)hipErrorInvalidValue;
  if (Q == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const long nrb = ((long)N + 4L * rows_per_wave - 1) / (4L * rows_per_wave);
  const int nrb8 = (int)((nrb + 7) / 8 * 8);
  const int nqb = (Q + 15) / 16, nqg = (Q + 63) / 64;  // query blocks of 16 / groups of 64
  if ((long)nrb8 * nqg > 0x7fffffffL) return (int)hipErrorInvalidValue;
  float* cs = (float*)ws;
  int* ci = (int*)(cs + (size_t)nrb8 * Q * K);
  // shared-tile kernel: one workgroup per CU over the whole shard (multiples of its 32-row LDS
  // tile), never more row blocks than the workspace holds
  const int rpb = (int)max(4L * rows_per_wave, ((long)N + 256 * 32 - 1) / (256 * 32) * 32);
  const long nrb_mq = ((long)N + rpb - 1) / rpb;
  const int nrb8_mq = (int)((nrb_mq + 7) / 8 * 8);
#define TDS8(NG)                                                                                           \
  do {                                                                                                     \
    if (nqb == 1)                                                                                          \
      topk_dense_stream8_kernel<2 * NG><<<nrb8, 256, 0, s>>>((const uint8_t*)codes, (const float*)scale, N, \
          (const int*)slots, (const bf16_t*)Qv, Q, (const unsigned*)bitmap, W, thr, K, rows_per_wave, 1, cs, ci); \
    else                                                                                                   \
      topk_dense_mq8_kernel<NG><<<nrb8_mq * nqg, 256, 0, s>>>((const uint8_t*)codes, (const float*)scale, N, \
          (const int*)slots, (const bf16_t*)Qv, Q, (const unsigned*)bitmap, W, thr, K, rpb, nqg, cs, ci);   \
  } while (0)
  switch (d) {
    case 128: TDS8(1); break;
    case 384: TDS8(3); break;
    case 768: TDS8(6); break;
    default: TDS8(8); break;
  }
#undef TDS8
  int err = (int)hipGetLastError();
  if (err) return err;
  return da_topk_merge(cs, ci, nqb == 1 ? nrb8 : nrb8_mq, Q, K, out_s, out_i, stream);
}

DA_EXPORT int da_topk_ranges8(const void* codes, const void* scale, int d, const void* slots, const void* Qv, int Q,
                              const void* ranges, const void* range_off, const void* bitmap, int W, float thr,
                              int K, int splits, int rows_per_split, void* ws, void* out_s, void* out_i,
                              void* stream) {
  if (d % 16 || d > 4096 || d < 16 || K < 1 || K > TK_MAX || splits < 1 || !codes || !scale ||
      ((uintptr_t)codes & 15))
    return (int)hipErrorInvalidValue;
  if (Q == 0) return 0;
  float* cs = (float*)ws;
  int* ci = (int*)(cs + (size_t)splits * Q * K);
  dim3 grid(splits, Q);
  topk_ranges8_kernel<<<grid, 256, 0, (hipStream_t)stream>>>((const uint8_t*)codes, (const float*)scale, d,
                                                            (const int*)slots, (const bf16_t*)Qv, Q,
                                                            (const int*)ranges, (const int*)range_off,
                                                            (const unsigned*)bitmap, W, thr, K, rows_per_split, cs,
                                                            ci);
  int err = (int)hipGetLastError();
  if (err) return err;
  return da_topk_merge(cs, ci, splits, Q, K, out_s, out_i, stream);
}
