// Top-K machinery shared by the vector index scans (vecsearch.hip: bf16 rows; vecsearch8.hip: fp8
// rows): the candidate order, the sorted-list merge of the query-major / ranges kernels, and the
// per-wave candidate lists of the streaming scans (TdWave).
#pragma once
#include "common.h"

#define TK_MAX 32

__device__ __forceinline__ bool better(float a, int ia, float b, int ib) {
  return a > b || (a == b && ia >= 0 && (ib < 0 || ia < ib));
}

// Merge 64 new candidates (one per lane: a/ia) into a running sorted top-K list held in LDS
// (best/bidx, K entries) — executed by one full wave.
__device__ __forceinline__ void wave_merge_topk(float a, int ia, float* best, int* bidx, int K, int lane) {
  const float kth = best[K - 1];
  const int kthi = bidx[K - 1];
  // early exit: nothing beats the current k-th
  const bool cand = better(a, ia, kth, kthi) && a != -INFINITY;
  if (__ballot(cand) == 0ull) return;
  float b = lane < K ? best[lane] : -INFINITY;
  int ib = lane < K ? bidx[lane] : -1;
  float outv = -INFINITY;
  int outi = -1;
  for (int r = 0; r < K; ++r) {
    // local best of (a, b)
    float v; int vi; int which;
    if (better(a, ia, b, ib)) { v = a; vi = ia; which = 0; } else { v = b; vi = ib; which = 1; }
    if (v == -INFINITY) { vi = -1; }
    float wv = v; int wi = vi; int wl = lane;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(wv, o, 64);
      const int oi = __shfl_xor(wi, o, 64);
      const int ol = __shfl_xor(wl, o, 64);
      if (better(ov, oi, wv, wi) || (ov == wv && oi == wi && ol < wl)) { wv = ov; wi = oi; wl = ol; }
    }
    if (lane == r) { outv = wv; outi = (wv == -INFINITY) ? -1 : wi; }
    if (lane == wl) {
      if (which == 0) { a = -INFINITY; ia = -1; } else { b = -INFINITY; ib = -1; }
    }
  }
  if (lane < K) { best[lane] = outv; bidx[lane] = outi; }
}

// One wave's top-K state for its 16 queries over a run of 16-row tiles. Per query, 64 LDS slots:
// [0, K) the current top-K (unsorted), then one candidate sub-buffer of SB slots for each of the
// query's 4 lanes; the k-th best score sits in a register of those lanes.
//  * tile(): a lane's rows that beat the k-th best pass the doc filter / floor and go to ITS
//    sub-buffer at a lane-local count: no cross-lane traffic on the append path.
//  * cut(): once a sub-buffer could overflow on the next tile, the query's list + buffered rows (one
//    per lane, <= 64) are cut to the top K by a radix select on the ballot unit: 32 rounds of ballot
//    + popcount on an order-preserving integer image of the score find the K-th largest (ties at
//    the threshold go to the smaller row id), the winners are compacted into [0, K) by mbcnt. The
//    sorted-list merge it replaces (K rounds of a 6-level shuffle argmax per (tile, query), then
//    per 48 candidates) stalled the workgroup's load pipeline: 64 queries took 10.5 ms against
//    3.7 ms with no candidate work (bench/scan_probe.py, profiles/r5/index/).
// Lists leave unsorted; topk_merge_kernel orders them.
constexpr int TD_SL = 64;  // LDS slots per (wave, query)

__device__ __forceinline__ unsigned td_key(float v, int id) {  // larger = better; empty (id < 0) = 0
  const unsigned u = __float_as_uint(v);
  return id < 0 ? 0u : ((u & 0x80000000u) ? ~u : (u | 0x80000000u));
}
__device__ __forceinline__ float td_unkey(unsigned k) {
  return k == 0u ? -INFINITY : __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ void wave_sync_lds() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The top K of the wave's 64 (v, id) (one per lane; id < 0 = empty) into cs/ci[0, K) of a list,
// unsorted. Returns the K-th best score (-inf while fewer than K are real). Every lane must have
// read what it passes before the call (the list slots are overwritten).
__device__ __forceinline__ float td_cut(float v, int id, int K, int lane, float* cs, int* ci) {
  const unsigned key = td_key(v, id);
  unsigned T = 0;  // the K-th largest key (empty lanes have key 0)
  int need = K;
  bool act = true;
  for (int bt = 31; bt >= 0; --bt) {
    const bool one = (key >> bt) & 1u;
    const int c1 = __popcll(__ballot(act && one));
    if (c1 >= need) { T |= 1u << bt; act = act && one; }
    else { need -= c1; act = act && !one; }
  }
  // winners: every key > T, then `need` of the keys == T (smallest row ids; empties: any)
  unsigned long long sel = __ballot(key > T);
  unsigned long long eq = __ballot(key == T);
  need = K - __popcll(sel);
  if (__popcll(eq) <= need || T == 0u) {
    for (; need > 0 && eq; --need) { sel |= eq & (~eq + 1); eq &= eq - 1; }
  } else {  // exact score ties at the threshold (rare): smallest row ids first
    for (; need > 0; --need) {
      int m = ((eq >> lane) & 1ull) ? id : 0x7fffffff;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o, 64));
      const unsigned long long w = __ballot(((eq >> lane) & 1ull) && id == m);
      sel |= w & (~w + 1);
      eq &= ~(w & (~w + 1));
    }
  }
  const int pos = __builtin_amdgcn_mbcnt_hi((unsigned)(sel >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)sel, 0u));
  wave_sync_lds();
  if ((sel >> lane) & 1ull) { cs[pos] = v; ci[pos] = id; }
  wave_sync_lds();
  return td_unkey(T);
}

struct TdWave {
  float* cs; int* ci;  // [16][TD_SL] scores / rows
  int K, SB, lane, fr, fg;
  float kth;  // this lane's query (fr): its current k-th best score
  int cnt;    // entries in this lane's sub-buffer

  __device__ __forceinline__ void init(float* s, int* i, int k) {
    cs = s; ci = i; K = k; SB = (TD_SL - k) / 4;  // K <= 32: SB >= 8
    lane = threadIdx.x & 63; fr = lane & 15; fg = lane >> 4;
    kth = -INFINITY; cnt = 0;
    for (int j = lane; j < 16 * TD_SL; j += 64) { cs[j] = -INFINITY; ci[j] = -1; }
  }
  // cut the lists of the queries set in `full` (bit q) back to their top K
  __device__ __forceinline__ void flush(const unsigned long long full) {
    wave_sync_lds();
    float kq = -INFINITY;  // lane q < 16: query q's new k-th best
    for (unsigned long long left = full; left; left &= left - 1) {
      const int q = __builtin_ctzll(left);
      // lane j: list slot j (< K) or sub-buffer b = (j - K) / SB entry (j - K) % SB, live below the
      // count of lane q + 16 b
      const int b = lane < K ? 0 : min((lane - K) / SB, 3), e = lane < K ? 0 : lane - K - b * SB;
      const int nb = __shfl(cnt, q + 16 * b, 64);
      const bool live = lane < K || (lane < K + 4 * SB && e < nb);
      const float v = live ? cs[q * TD_SL + lane] : -INFINITY;
      const int id = live ? ci[q * TD_SL + lane] : -1;
      const float t = td_cut(v, id, K, lane, cs + q * TD_SL, ci + q * TD_SL);
      if (lane == q) kq = t;
    }
    const float kn = __shfl(kq, fr, 64);
    if ((full >> fr) & 1ull) { kth = kn; cnt = 0; }
  }
  // a finished 16 x 16 tile: lane (fr, fg) holds rows row0 + i (row0 = tile base + 4 fg) of query fr
  // (global query index qrow); rows from `end` on are padding
  __device__ __forceinline__ void tile(const f32x4_t& acc, int row0, int end, bool qok, float thr,
                                       const int* __restrict__ slots, const unsigned* __restrict__ bitmap, int W,
                                       int qrow) {
    bool cand = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) cand |= qok && row0 + i < end && acc[i] >= thr && acc[i] > kth;
    if (!__ballot(cand)) return;  // the common case after the first tiles
    float* bs = cs + fr * TD_SL + K + fg * SB;
    int* bi = ci + fr * TD_SL + K + fg * SB;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = row0 + i;
      bool ok = qok && row < end && acc[i] >= thr && acc[i] > kth;
      if (ok && slots) {  // removed rows (slot -1) never match; the bitmap filters documents
        const int sl = slots[row];
        ok = sl >= 0 && (!bitmap || ((sl >> 5) < W && ((bitmap[(size_t)qrow * W + (sl >> 5)] >> (sl & 31)) & 1u)));
      }
      if (ok) { bs[cnt] = acc[i]; bi[cnt] = row; ++cnt; }
    }
    // a lane's next tile adds <= 4: cut the queries with a sub-buffer past SB - 4
    const unsigned long long over = __ballot(cnt > SB - 4);
    if (over) flush((over | (over >> 16) | (over >> 32) | (over >> 48)) & 0xffffull);
  }
  // every list cut to its top K (unsorted) in slots [0, K)
  __device__ __forceinline__ void finish() {
    const unsigned long long rest = __ballot(cnt > 0);
    if (rest) flush((rest | (rest >> 16) | (rest >> 32) | (rest >> 48)) & 0xffffull);
  }
  // merge another wave's finished lists (same 16 queries) into this wave's
  __device__ __forceinline__ void absorb(const float* os, const int* oi, int nq) {
    wave_sync_lds();
    for (int q = 0; q < nq; ++q) {
      const float v = lane < K ? cs[q * TD_SL + lane] : lane < 2 * K ? os[q * TD_SL + lane - K] : -INFINITY;
      const int id = lane < K ? ci[q * TD_SL + lane] : lane < 2 * K ? oi[q * TD_SL + lane - K] : -1;
      td_cut(v, id, K, lane, cs + q * TD_SL, ci + q * TD_SL);
    }
  }
  // lists of queries [0, nq) -> out[o0 + q * K + j] (o0: this list's (part, first query) offset)
  __device__ __forceinline__ void store(int nq, size_t o0, float* __restrict__ os, int* __restrict__ oi) {
    wave_sync_lds();
    for (int i = lane; i < nq * K; i += 64) {
      const int q = i / K, j = i % K;
      os[o0 + i] = cs[q * TD_SL + j];
      oi[o0 + i] = ci[q * TD_SL + j];
    }
  }
};
