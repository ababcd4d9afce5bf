// Flash prefill attention for gfx950 (decode attention: decode_attn.hip).
//
// flash_attn_v2: packed (varlen) prefill attention, bidirectional (BERT encoder)
// or causal with GQA (Llama-3 / Phi-3 prefill, N6/N7), optionally over a shared-prefix head in
// the KV cache. Online softmax in fp32, bf16 MFMA 32x32x16, "swapped" S^T = K.Q^T formulation
// (details above the kernel). flash_attn_pipe: the same math, software-pipelined, for the causal
// D = 96 prefill.
#include "common.h"

// Floating-point contraction only within one expression (a*b + c -> fma), never across statements:
// with the HIP default (fast) the backend fuses differently depending on the code around an
// expression. Pinned, the bits of an expression do not depend on the surrounding code, so the
// pipelined kernel, the tail-only launch and flash_attn_v2 round the same math alike.
#pragma clang fp contract(on)

// ------------------------------------------------------------------------------------------
// flash_attn_v2: 32x32x16 MFMA, 4 waves x 32 queries (128 queries per workgroup), 64-key tiles
// double-buffered in LDS with register staging (tile t+1's global loads are in flight while tile t
// is computed; one barrier per tile).
//   S^T[key][q] = K·Q^T : A = K rows from LDS (16-B pad per row -> conflict-free ds_read_b128),
//                         B = Q^T from registers (loaded once per wave).
//   lane l owns query l&31; its 32 keys of a 64-key tile sit in the two S^T accumulators, the
//   other 32 in lane l^32 -> row max / row sum need ONE v_permlane32_swap each.
//   O^T[d][q] += V^T·P^T : B = P^T straight from the S^T registers (k index permuted), A = V^T
//                         fetched from the row-major V tile with ds_read_b64_tr_b16 (hardware
//                         transpose; row stride chosen so the 4-row x 2-group reads are
//                         bank-conflict-free).
//   scale·log2(e) is folded into the exp2 argument (one FMA per score); the O rescale is skipped
//   when no lane's running max moved; causal tiles past a wave's last query are skipped by that
//   wave (it still stages tiles and joins the barrier).
template <int D, int NW = 4, int QH = 1>
struct FA2Cfg {
  static constexpr int KT = 64, QW = 32 * QH, QB = QW * NW, NT = 64 * NW;
  static constexpr int KSTR = D * 2 + 16;                                         // bytes
  static constexpr int VSTR = (D == 64) ? 192 : (D == 128) ? 320 : D * 2;         // bytes
  static constexpr int KBUF = KT * KSTR, VBUF = KT * VSTR;
  static constexpr int CPR = D / 8, LPT = (KT * CPR + NT - 1) / NT;
  static constexpr int SMEM = 2 * (KBUF + VBUF);
};

// Shared-prefix keys (pre.len > 0): every sequence's keys are [pre.len prefix keys | its own keys];
// the prefix K/V live once in a KV-cache slot ([Hkv][max_seq][D]: head stride pre.hstride, row
// stride D), RoPE already applied. Query i of a sequence sits at key position pre.len + i (causal
// mask bottom-right aligned), so a batch whose prompts share a system-prompt head prefills that
// head once and only the suffixes here.
struct FaPrefix {
  const bf16_t* k;
  const bf16_t* v;
  long long hstride;
  int len;
  int rev;  // dispatch order (set by the launcher): bit 0 causal longest-first, bit 1 XCD-grouped
  // own keys from the KV cache (pipelined D = 96 kernel; null: from the k / v views): sequence b's
  // keys at cache[kv_slot[cu[b]], hk, kv_pos[cu[b]] + j, :] (slot_stride = Hkv * max_seq * D,
  // head stride hstride), rows D apart — the QKV epilogue then stores k / v to the cache only
  const int* kv_slot;
  const int* kv_pos;
  const bf16_t* kc;
  const bf16_t* vc;
  long long slot_stride;
  // tail mode (grid x = 1): each (sequence, head) computes and stores only the query block that
  // holds the sequence's last token, exactly as the full launch computes that block (same q0, key
  // range, tiles, code path: the same bits); every other row of o is left unwritten
  int tail;
};

// The (query block, head, sequence) a flash workgroup works on, from its place in the dispatch
// order. rev bit 0 (causal): the longest query blocks (most keys) first, so the kernel's tail is
// made of short blocks (longest-processing-time-first packing). rev bit 1: the query blocks of one
// (sequence, kv head) pair all run on one XCD. Workgroups are dealt round-robin over the 8 XCDs
// (linear ids g and g + 8 share one: observed dispatch, relied on for speed only), and every block
// of a pair re-reads that pair's K / V rows; grid order put a pair's blocks on all 8 XCDs, so each
// XCD's L2 fetched the same rows. Grouped, the pair's rows are fetched into one L2 and re-read
// there (pair-major per XCD: a few pairs' rows live at a time).
struct FaBlock {
  int qb, h, b;
};
__device__ __forceinline__ FaBlock fa_block(int rev, int causal, int G) {
  const int X = gridDim.x, Y = gridDim.y, Z = gridDim.z;
  const bool lpt = causal && (rev & 1);
  if ((rev & 2) && G >= 1 && Y % G == 0 && ((Y / G) * Z) % 8 == 0) {
    const int g = blockIdx.x + X * (blockIdx.y + Y * blockIdx.z);
    const int xcd = g & 7, s = g >> 3;
    const int per = X * G;                         // workgroups of one (sequence, kv head) pair
    const int pair = (s / per) * 8 + xcd, r = s % per;
    const int qi = r / G, gh = r % G;               // all G heads' longest blocks first
    const int hkv = Y / G;
    return FaBlock{lpt ? X - 1 - qi : qi, (pair % hkv) * G + gh, pair / hkv};
  }
  return FaBlock{lpt ? X - 1 - (int)blockIdx.x : (int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z};
}

// The query block a workgroup runs: its place in the dispatch order, or in tail mode the block (of
// QB rows) that holds the last token of its sequence (L tokens; the grid is one block wide, so
// fa_block's XCD grouping sees per = G workgroups per pair and its longest-first order one block).
__device__ __forceinline__ int fa_query_block(const FaBlock& fb, int tail, int L, int QB) {
  return tail ? (L > 0 ? (L - 1) / QB : 0) : fb.qb;
}

// QH = 32-query halves per wave. QH = 2: each K fragment read from LDS feeds the S MFMAs of both
// halves and each transposed V fragment the O MFMAs of both, so LDS read bytes per FLOP halve (at
// QH = 1 the LDS reads of a tile take as long as its MFMAs); the two halves' softmax VALU work is
// independent of the other half's MFMAs, so the scheduler overlaps them inside one wave.
template <int D, int NW, int QH, typename T = BF16T>
__global__ void __launch_bounds__(64 * NW, QH == 1 ? 8 / NW : 1)
flash_attn_v2_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
                     int ldq, int ldk, int ldv, const int* __restrict__ cu, int H, int Hkv, int causal,
                     float c, bf16_t* __restrict__ o, int ldo, FaPrefix pre) {
  using C = FA2Cfg<D, NW, QH>;
  constexpr int KT = C::KT, NDS = D / 16, NDB = D / 32, CPR = C::CPR, LPT = C::LPT, NT = C::NT;
  constexpr bool EVEN = (KT * CPR) % NT == 0;  // every thread stages exactly LPT chunks
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const FaBlock fb = fa_block(pre.rev, causal, H / Hkv);  // dispatch order: see fa_block
  const int b = fb.b, h = fb.h;
  const int s0 = cu[b], L = cu[b + 1] - s0;
  const int qb = fa_query_block(fb, pre.tail, L, C::QB);
  const int q0 = qb * C::QB;
  if (q0 >= L) return;
  const int hk = h / (H / Hkv);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int qr = lane & 31, hi = lane >> 5;
  const int wq0 = q0 + wid * C::QW;
  int qi[QH];
  bool qvalid[QH];
  bf16x8_t qf[QH][NDS];
  f32x16_t oacc[QH][NDB];
  float m_run[QH], l_part[QH];
#pragma unroll
  for (int j = 0; j < QH; ++j) {
    qi[j] = wq0 + 32 * j + qr;
    qvalid[j] = qi[j] < L;
#pragma unroll
    for (int ds = 0; ds < NDS; ++ds) {
      if (qvalid[j]) qf[j][ds] = *(const bf16x8_t*)(q + (size_t)(s0 + qi[j]) * ldq + h * D + ds * 16 + hi * 8);
      else qf[j][ds] = bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0};
    }
#pragma unroll
    for (int i = 0; i < NDB; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[j][i][r] = 0.f;
    m_run[j] = -INFINITY;
    l_part[j] = 0.f;
  }

  const int P = pre.len, Lk = P + L;  // keys: [prefix | own]; own query i is key P + i
  const int kv_end = causal ? min(Lk, P + q0 + C::QB) : Lk;
  const int wave_end = causal ? min(Lk, P + wq0 + C::QW) : Lk;
  const int ntiles = (kv_end + KT - 1) / KT;

  const bf16_t* kbase_p = k + (size_t)s0 * ldk + hk * D;
  const bf16_t* vbase_p = v + (size_t)s0 * ldv + hk * D;
  if (pre.kv_slot) {  // own keys in the cache (the launcher passes ldk = ldv = D)
    const size_t off = (size_t)pre.kv_slot[s0] * pre.slot_stride + (size_t)hk * pre.hstride + (size_t)pre.kv_pos[s0] * D;
    kbase_p = pre.kc + off;
    vbase_p = pre.vc + off;
  }
  const bf16_t* kpre = pre.k + hk * pre.hstride;
  const bf16_t* vpre = pre.v + hk * pre.hstride;
  u32x4_t kst[LPT], vst[LPT];
  // Own-key tiles (all keys >= P) load through buffer resources rebuilt per tile on the scalar unit
  // (base = the tile's first key, num_records = the bytes left in the sequence: keys past the end
  // read 0), with fixed per-lane 32-bit offsets: no per-load 64-bit address math, bounds compare or
  // exec-mask branch (those were ~90 of the ~285 vector instructions of a tile).
  unsigned koff[LPT], voff[LPT];
#pragma unroll
  for (int i = 0; i < LPT; ++i) {
    const int idx = tid + NT * i, r = idx / CPR, cc = idx % CPR;
    const bool in = EVEN || idx < KT * CPR;
    koff[i] = in ? (unsigned)(r * ldk * 2 + cc * 16) : 0x80000000u;
    voff[i] = in ? (unsigned)(r * ldv * 2 + cc * 16) : 0x80000000u;
  }
  auto load_tile = [&](int t) {
    const int k0 = t * KT;
    if (k0 >= P) {
      const int o0 = k0 - P;
      const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(kbase_p + (size_t)o0 * ldk), (short)0, (L - o0) * ldk * 2, 0x00020000);
      const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(vbase_p + (size_t)o0 * ldv), (short)0, (L - o0) * ldv * 2, 0x00020000);
#pragma unroll
      for (int i = 0; i < LPT; ++i) {
        kst[i] = __builtin_amdgcn_raw_buffer_load_b128(rk, koff[i], 0, 0);
        vst[i] = __builtin_amdgcn_raw_buffer_load_b128(rv, voff[i], 0, 0);
      }
      return;
    }
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      const int idx = tid + NT * i, r = idx / CPR, cc = idx % CPR, key = t * KT + r;
      if ((EVEN || idx < KT * CPR) && key < Lk) {
        if (key >= P) {
          kst[i] = *(const u32x4_t*)(kbase_p + (size_t)(key - P) * ldk + cc * 8);
          vst[i] = *(const u32x4_t*)(vbase_p + (size_t)(key - P) * ldv + cc * 8);
        } else {
          kst[i] = *(const u32x4_t*)(kpre + (size_t)key * D + cc * 8);
          vst[i] = *(const u32x4_t*)(vpre + (size_t)key * D + cc * 8);
        }
      } else {
        kst[i] = u32x4_t{0, 0, 0, 0};
        vst[i] = u32x4_t{0, 0, 0, 0};
      }
    }
  };
  auto store_tile = [&](int buf) {
    char* sK = smem + buf * (C::KBUF + C::VBUF);
    char* sV = sK + C::KBUF;
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      const int idx = tid + NT * i, r = idx / CPR, cc = idx % CPR;
      if (EVEN || idx < KT * CPR) {
        *(u32x4_t*)(sK + r * C::KSTR + cc * 16) = kst[i];
        *(u32x4_t*)(sV + r * C::VSTR + cc * 16) = vst[i];
      }
    }
  };

  load_tile(0);
  store_tile(0);
  __syncthreads();

  for (int t = 0; t < ntiles; ++t) {
    const int cur = t & 1;
    if (t + 1 < ntiles) load_tile(t + 1);
    const int kb = t * KT;
    if (kb < wave_end) {
      const char* sK = smem + cur * (C::KBUF + C::VBUF);
      const char* sV = sK + C::KBUF;
      f32x16_t sacc[QH][2];
      // all K fragments of the tile first, then the MFMAs with the two 32-key halves interleaved:
      // one LDS round trip per tile instead of one per MFMA, and back-to-back MFMAs never depend
      // on each other (a fragment-at-a-time loop serialises LDS latency + MFMA latency 12 times).
      // D = 128 (16 fragments) batches per 32-key half, which keeps it within 256 VGPRs.
#pragma unroll
      for (int j = 0; j < QH; ++j)
#pragma unroll
        for (int hh = 0; hh < 2; ++hh)
#pragma unroll
          for (int r = 0; r < 16; ++r) sacc[j][hh][r] = 0.f;
      if constexpr (NDS <= 6) {
        bf16x8_t kfr[2][NDS];
#pragma unroll
        for (int hh = 0; hh < 2; ++hh)
#pragma unroll
          for (int ds = 0; ds < NDS; ++ds)
            kfr[hh][ds] = *(const bf16x8_t*)(sK + (hh * 32 + qr) * C::KSTR + ds * 32 + hi * 16);
#pragma unroll
        for (int ds = 0; ds < NDS; ++ds)
#pragma unroll
          for (int hh = 0; hh < 2; ++hh)
#pragma unroll
            for (int j = 0; j < QH; ++j) sacc[j][hh] = T::mma32(kfr[hh][ds], qf[j][ds], sacc[j][hh]);
        // pin that order: the register-pressure scheduler otherwise re-serialises read -> MFMA pairs
        __builtin_amdgcn_sched_group_barrier(0x100, 2 * NDS, 0);       // DS reads
        __builtin_amdgcn_sched_group_barrier(0x008, 2 * NDS * QH, 0);  // MFMAs
      } else {
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
          bf16x8_t kfr[NDS];
#pragma unroll
          for (int ds = 0; ds < NDS; ++ds)
            kfr[ds] = *(const bf16x8_t*)(sK + (hh * 32 + qr) * C::KSTR + ds * 32 + hi * 16);
#pragma unroll
          for (int ds = 0; ds < NDS; ++ds)
#pragma unroll
            for (int j = 0; j < QH; ++j) sacc[j][hh] = T::mma32(kfr[ds], qf[j][ds], sacc[j][hh]);
          __builtin_amdgcn_sched_group_barrier(0x100, NDS, 0);
          __builtin_amdgcn_sched_group_barrier(0x008, NDS * QH, 0);
        }
      }
#pragma unroll
      for (int j = 0; j < QH; ++j) {
        if (kb + KT > Lk || (causal && kb + KT - 1 > P + wq0 + 32 * j)) {
#pragma unroll
          for (int hh = 0; hh < 2; ++hh)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int key = kb + hh * 32 + 8 * (r >> 2) + 4 * hi + (r & 3);
              if (key >= Lk || (causal && key > P + qi[j])) sacc[j][hh][r] = -INFINITY;
            }
        }
        float mx = sacc[j][0][0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = fmaxf(mx, sacc[j][0][r]);
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sacc[j][1][r]);
        mx = max_xhalf(mx);
        const float m_new = fmaxf(m_run[j], mx);
        const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
        if (__any(m_new > m_run[j])) {
          const float alpha = exp2f((m_run[j] - m_use) * c);
          l_part[j] *= alpha;
#pragma unroll
          for (int i = 0; i < NDB; ++i) oacc[j][i] *= alpha;
        }
        m_run[j] = m_new;
        const float mc = -m_use * c;
        float psum = 0.f;
#pragma unroll
        for (int hh = 0; hh < 2; ++hh)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float p = __builtin_amdgcn_exp2f(fmaf(sacc[j][hh][r], c, mc));  // raw v_exp_f32
            sacc[j][hh][r] = p;
            psum += p;
          }
        l_part[j] += psum;
      }

      // O^T += V^T P^T over 4 k-steps of 16 keys: slot (hi, j) -> key 16kc + 8(j>>2) + 4hi + (j&3)
#pragma unroll
      for (int kc = 0; kc < 4; ++kc) {
        const int hh = kc >> 1, cb = (kc & 1) * 8;
        bf16x8_t pb[QH];
#pragma unroll
        for (int j = 0; j < QH; ++j) {
          const u32x4_t pw = u32x4_t{T::pack2(sacc[j][hh][cb], sacc[j][hh][cb + 1]),
                                     T::pack2(sacc[j][hh][cb + 2], sacc[j][hh][cb + 3]),
                                     T::pack2(sacc[j][hh][cb + 4], sacc[j][hh][cb + 5]),
                                     T::pack2(sacc[j][hh][cb + 6], sacc[j][hh][cb + 7])};
          pb[j] = __builtin_bit_cast(bf16x8_t, pw);
        }
        const int g = lane >> 4, li = lane & 15;
        const int row0 = kc * 16 + 4 * (g >> 1) + (li >> 2);
#pragma unroll
        for (int db = 0; db < NDB; ++db) {
          const int col = db * 32 + 16 * (g & 1) + 4 * (li & 3);
          const s16x4_t lo = lds_read_tr16(sV + row0 * C::VSTR + col * 2);
          const s16x4_t hi8 = lds_read_tr16(sV + (row0 + 8) * C::VSTR + col * 2);
          const bf16x8_t va = bf16x8_t{lo[0], lo[1], lo[2], lo[3], hi8[0], hi8[1], hi8[2], hi8[3]};
#pragma unroll
          for (int j = 0; j < QH; ++j) oacc[j][db] = T::mma32(va, pb[j], oacc[j][db]);
        }
      }
    }
    if (t + 1 < ntiles) store_tile(cur ^ 1);
    __syncthreads();
  }

#pragma unroll
  for (int j = 0; j < QH; ++j) {
    const float l_tot = sum_xhalf(l_part[j]);
    const float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
    if (qvalid[j]) {
      bf16_t* orow = o + (size_t)(s0 + qi[j]) * ldo + h * D;
#pragma unroll
      for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int d = db * 32 + 8 * g + 4 * hi;
          *(u32x2_t*)(orow + d) = u32x2_t{T::pack2(oacc[j][db][4 * g] * inv, oacc[j][db][4 * g + 1] * inv),
                                          T::pack2(oacc[j][db][4 * g + 2] * inv, oacc[j][db][4 * g + 3] * inv)};
        }
    }
  }
}

// ------------------------------------------------------------------------------------------
// flash_attn_pipe: the same math and fragment layouts as flash_attn_v2<D, 4, 1>, software-pipelined
// one tile deep (guide T15): the S MFMAs of tile t + 1 are issued before the softmax + P·V of tile t,
// so the softmax VALU work never waits on the MFMA results it follows (RAW) and the matrix pipe has
// independent work while a wave is in its exp/max/pack stretch. Three LDS tile buffers: tile t
// (P·V), t + 1 (S) and t + 2 (being written); one barrier per tile.
//
// SPEC = true: speculative softmax against a deferred running max (guide T13). The round-2 form put
// the S MFMAs of tile t + 1, the max / rescale branch and the exp / pack / P·V of tile t in separate
// basic blocks, so the compiler could not interleave the softmax VALU of t with the S MFMAs of t + 1
// (ISA: a 12-MFMA block with no VALU, then a 116-VALU + 32-exp block; the SIMD ran them back to back).
// With SPEC, an unmasked tile (every key visible to every query of the wave) is one straight-line
// block: S(t + 1) MFMAs interleaved with max(t), p = exp2(s·c - m_run·c) against the STALE running
// max, row sums and the bf16 pack. The reference max of a query moves only when its tile max
// overshoots it by SPEC_TAU (log2 units of p; the first tile always does), branch-free per lane;
// only the O rescale that such a move needs is a (rare, wave-uniform) branch before P·V. Masked
// tiles (causal diagonal, sequence end) take the exact path. p <= 2^SPEC_TAU keeps the fp32 sums
// and the bf16 P exact in relative terms; the result is normalised by the same l, so only rounding
// differs from SPEC = false.
//
// DMA = true (D = 96, shared prefix a multiple of 64 keys): K / V tiles arrive by LDS-DMA
// (buffer_load ... lds) instead of register staging, in rings that give each tile TWO steps of
// latency cover (staging gave one, and a step is ~0.5 us against 1-2 us of loaded HBM / L2
// latency): at the start of step t the wave issues K(t + 3) into the slot S(t) read in step t - 1
// and V(t + 2) into the slot P·V(t - 1) read; before the step's barrier it waits for K(t + 2) and
// V(t + 1) (vmcnt(6): the 3 + 3 pieces of step t may stay in flight). K rows are unpadded (192 B)
// with 16-B chunk c of row r at slot c ^ ((r >> 2) & 3) — applied on the DMA source side — so the
// 16 rows one ds_read_b128 lane group reads hit 16 distinct bank slots; V keeps its linear rows.
// No staging registers, no ds_write, no per-tile address VALU. Past the last tile the pieces are
// issued at an out-of-range offset (no memory traffic, zeros into a free slot): uniform counts.
constexpr float SPEC_TAU = 8.f;

// Three 1-KiB LDS-DMA pieces (buffer_load_dwordx4 ... lds) into LDS lds, lds + 1 KiB, lds + 2 KiB,
// lane l's 16 B from rsrc + v_i + soff. Inline asm on purpose: through the builtin, hipcc treats the
// transposed V reads (ds_read_b64_tr_b16) as possibly aliasing the DMA and drains vmcnt to 0 before
// them, which would cancel the prefetch; these ops are invisible to its counters, and the kernel
// waits for them with explicit vmcnt. No VGPR destination (register-safe); M0 is saved and
// restored inside the statement; s_nop 4 covers an SGPR operand fresh from v_readfirstlane.
__device__ __forceinline__ void dma3_lds(__amdgpu_buffer_rsrc_t rs, unsigned lds, unsigned v0, unsigned v1,
                                         unsigned v2, int soff) {
  unsigned keep;
  asm volatile(
      "s_nop 4\n\t"
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %5\n\t"
      "s_nop 0\n\t"
      "buffer_load_dwordx4 %1, %4, %6 offen lds\n\t"
      "s_add_u32 m0, m0, 0x400\n\t"
      "s_nop 0\n\t"
      "buffer_load_dwordx4 %2, %4, %6 offen lds\n\t"
      "s_add_u32 m0, m0, 0x400\n\t"
      "s_nop 0\n\t"
      "buffer_load_dwordx4 %3, %4, %6 offen lds\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(v0), "v"(v1), "v"(v2), "s"(rs), "s"(lds), "s"(soff)
      : "memory", "scc");
}

template <int D, bool SPEC, bool DMA>
__global__ void __launch_bounds__(256, 2)
flash_attn_pipe_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
                       int ldq, int ldk, int ldv, const int* __restrict__ cu, int H, int Hkv, int causal,
                       float c, bf16_t* __restrict__ o, int ldo, FaPrefix pre) {
  using C = FA2Cfg<D, 4, 1>;
  constexpr int KT = C::KT, NDS = D / 16, NDB = D / 32, CPR = C::CPR, LPT = C::LPT, NT = C::NT;
  constexpr bool EVEN = (KT * CPR) % NT == 0;
  static_assert(NDS <= 6, "pipelined flash: D <= 96");
  static_assert(!DMA || (D == 96 && C::VSTR == D * 2), "DMA tiles: D = 96 (linear V rows)");
  constexpr int KSTR = DMA ? D * 2 : C::KSTR, KBUF = KT * KSTR, TBUF = KBUF + C::VBUF;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const FaBlock fb = fa_block(pre.rev, causal, H / Hkv);  // dispatch order: see fa_block
  const int b = fb.b, h = fb.h;
  const int s0 = cu[b], L = cu[b + 1] - s0;
  const int qb = fa_query_block(fb, pre.tail, L, C::QB);
  const int q0 = qb * C::QB;
  if (q0 >= L) return;
  const int hk = h / (H / Hkv);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int qr = lane & 31, hi = lane >> 5;
  const int wq0 = q0 + wid * C::QW;
  const int qi = wq0 + qr;
  const bool qvalid = qi < L;
  bf16x8_t qf[NDS];
#pragma unroll
  for (int ds = 0; ds < NDS; ++ds)
    qf[ds] = qvalid ? *(const bf16x8_t*)(q + (size_t)(s0 + qi) * ldq + h * D + ds * 16 + hi * 8)
                    : bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0};
  f32x16_t oacc[NDB];
#pragma unroll
  for (int i = 0; i < NDB; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[i][r] = 0.f;
  float m_run = -INFINITY, l_part = 0.f;

  const int P = pre.len, Lk = P + L;
  const int kv_end = causal ? min(Lk, P + q0 + C::QB) : Lk;
  const int wave_end = causal ? min(Lk, P + wq0 + C::QW) : Lk;
  const int ntiles = (kv_end + KT - 1) / KT;

  const bf16_t* kbase_p = k + (size_t)s0 * ldk + hk * D;
  const bf16_t* vbase_p = v + (size_t)s0 * ldv + hk * D;
  if (pre.kv_slot) {  // own keys in the cache (the launcher passes ldk = ldv = D)
    const size_t off = (size_t)pre.kv_slot[s0] * pre.slot_stride + (size_t)hk * pre.hstride + (size_t)pre.kv_pos[s0] * D;
    kbase_p = pre.kc + off;
    vbase_p = pre.vc + off;
  }
  const bf16_t* kpre = pre.k + hk * pre.hstride;
  const bf16_t* vpre = pre.v + hk * pre.hstride;
  auto buf_of = [&](int t) { return smem + (t % 3) * TBUF; };
  u32x4_t kst[LPT], vst[LPT];
  unsigned koff[LPT], voff[LPT];
#pragma unroll
  for (int i = 0; i < LPT; ++i) {
    const int idx = tid + NT * i, r = idx / CPR, cc = idx % CPR;
    const bool in = EVEN || idx < KT * CPR;
    koff[i] = in ? (unsigned)(r * ldk * 2 + cc * 16) : 0x80000000u;
    voff[i] = in ? (unsigned)(r * ldv * 2 + cc * 16) : 0x80000000u;
  }
  // DMA pieces: wave wid fills LDS 16-B positions (3 wid + i) * 64 + lane of a tile (768 = 64 rows x
  // 12 chunks): row r, slot sl; K slot sl holds chunk sl ^ ((r >> 2) & 3), V slot sl chunk sl
  unsigned dkr[3], dkc[3], dvc[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int pos = (wid * 3 + i) * 64 + lane, r = pos / 12, sl = pos % 12;
    dkr[i] = r;
    dkc[i] = (sl ^ ((r >> 2) & 3)) * 16;
    dvc[i] = sl * 16;
  }
  // tile t's K (KV = false) or V pieces into slot t % 3; t >= ntiles: out of range, no traffic
  auto dma_tile = [&](int t, bool is_v) {
    const int k0 = t * KT;
    const bf16_t* base = is_v ? vbase_p : kbase_p;
    const bf16_t* pbase = is_v ? vpre : kpre;
    const int ld = is_v ? ldv : ldk;
    const bool own = k0 >= P;
    const int o0 = k0 - P;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(own ? base + (size_t)o0 * ld : pbase + (size_t)k0 * D), (short)0,
        own ? max(L - o0, 0) * ld * 2 : (P - k0) * D * 2, 0x00020000);
    const unsigned rstride = own ? ld * 2 : D * 2;
    const int soff = t < ntiles ? 0 : 0x7ffffff0;
    typedef __attribute__((address_space(3))) char lds_char;  // LDS byte offset, not the flat address
    const unsigned dst = (unsigned)(size_t)(lds_char*)(buf_of(t) + (is_v ? KBUF : 0)) + wid * 3 * 1024;
    dma3_lds(rs, __builtin_amdgcn_readfirstlane(dst), dkr[0] * rstride + (is_v ? dvc[0] : dkc[0]),
             dkr[1] * rstride + (is_v ? dvc[1] : dkc[1]), dkr[2] * rstride + (is_v ? dvc[2] : dkc[2]), soff);
  };
  auto load_tile = [&](int t) {
    const int k0 = t * KT;
    if (k0 >= P) {
      const int o0 = k0 - P;
      const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(kbase_p + (size_t)o0 * ldk), (short)0, (L - o0) * ldk * 2, 0x00020000);
      const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(vbase_p + (size_t)o0 * ldv), (short)0, (L - o0) * ldv * 2, 0x00020000);
#pragma unroll
      for (int i = 0; i < LPT; ++i) {
        kst[i] = __builtin_amdgcn_raw_buffer_load_b128(rk, koff[i], 0, 0);
        vst[i] = __builtin_amdgcn_raw_buffer_load_b128(rv, voff[i], 0, 0);
      }
      return;
    }
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      const int idx = tid + NT * i, r = idx / CPR, cc = idx % CPR, key = t * KT + r;
      if ((EVEN || idx < KT * CPR) && key < Lk) {
        if (key >= P) {
          kst[i] = *(const u32x4_t*)(kbase_p + (size_t)(key - P) * ldk + cc * 8);
          vst[i] = *(const u32x4_t*)(vbase_p + (size_t)(key - P) * ldv + cc * 8);
        } else {
          kst[i] = *(const u32x4_t*)(kpre + (size_t)key * D + cc * 8);
          vst[i] = *(const u32x4_t*)(vpre + (size_t)key * D + cc * 8);
        }
      } else {
        kst[i] = u32x4_t{0, 0, 0, 0};
        vst[i] = u32x4_t{0, 0, 0, 0};
      }
    }
  };
  auto store_tile = [&](int t) {
    char* sK = buf_of(t);
    char* sV = sK + C::KBUF;
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      const int idx = tid + NT * i, r = idx / CPR, cc = idx % CPR;
      if (EVEN || idx < KT * CPR) {
        *(u32x4_t*)(sK + r * C::KSTR + cc * 16) = kst[i];
        *(u32x4_t*)(sV + r * C::VSTR + cc * 16) = vst[i];
      }
    }
  };
  // byte offset of K fragment (32-key half hh, 16-dim step ds) of this lane in a K tile
  auto kfrag = [&](int hh, int ds) -> int {
    if constexpr (DMA) return (hh * 32 + qr) * KSTR + (((2 * ds + hi) ^ ((qr >> 2) & 3)) << 4);
    else return (hh * 32 + qr) * KSTR + ds * 32 + hi * 16;
  };
  // S^T of tile t: all K fragments, then the MFMAs (two independent accumulation chains)
  auto s_tile = [&](int t, f32x16_t (&sa)[2]) {
    const char* sK = buf_of(t);
#pragma unroll
    for (int hh = 0; hh < 2; ++hh)
#pragma unroll
      for (int r = 0; r < 16; ++r) sa[hh][r] = 0.f;
    if constexpr (SPEC) {
      // one 32-key half at a time: 6 fragments (24 VGPRs) live instead of 12 beside the softmax of t
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        bf16x8_t kfr[NDS];
#pragma unroll
        for (int ds = 0; ds < NDS; ++ds)
          kfr[ds] = *(const bf16x8_t*)(sK + kfrag(hh, ds));
#pragma unroll
        for (int ds = 0; ds < NDS; ++ds) sa[hh] = mfma32(kfr[ds], qf[ds], sa[hh]);
      }
    } else {
      bf16x8_t kfr[2][NDS];
#pragma unroll
      for (int hh = 0; hh < 2; ++hh)
#pragma unroll
        for (int ds = 0; ds < NDS; ++ds)
          kfr[hh][ds] = *(const bf16x8_t*)(sK + kfrag(hh, ds));
#pragma unroll
      for (int ds = 0; ds < NDS; ++ds)
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) sa[hh] = mfma32(kfr[hh][ds], qf[ds], sa[hh]);
    }
  };
  // O^T += V^T P^T of tile t, P packed to bf16 (kc = 16-key step)
  auto pv_tile = [&](int t, const u32x4_t (&pw)[4]) {
    const char* sV = buf_of(t) + KBUF;
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) {
      const bf16x8_t pb = __builtin_bit_cast(bf16x8_t, pw[kc]);
      const int g = lane >> 4, li = lane & 15;
      const int row0 = kc * 16 + 4 * (g >> 1) + (li >> 2);
#pragma unroll
      for (int db = 0; db < NDB; ++db) {
        const int col = db * 32 + 16 * (g & 1) + 4 * (li & 3);
        const s16x4_t lo = lds_read_tr16(sV + row0 * C::VSTR + col * 2);
        const s16x4_t hi8 = lds_read_tr16(sV + (row0 + 8) * C::VSTR + col * 2);
        const bf16x8_t va = bf16x8_t{lo[0], lo[1], lo[2], lo[3], hi8[0], hi8[1], hi8[2], hi8[3]};
        oacc[db] = mfma32(va, pb, oacc[db]);
      }
    }
  };
  // mask + online softmax + O^T += V^T P^T of tile t
  auto finish = [&](int t, f32x16_t (&sa)[2]) {
    const int kb = t * KT;
    if (kb + KT > Lk || (causal && kb + KT - 1 > P + wq0)) {
#pragma unroll
      for (int hh = 0; hh < 2; ++hh)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = kb + hh * 32 + 8 * (r >> 2) + 4 * hi + (r & 3);
          if (key >= Lk || (causal && key > P + qi)) sa[hh][r] = -INFINITY;
        }
    }
    float mx = sa[0][0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, sa[0][r]);
#pragma unroll
    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sa[1][r]);
    mx = max_xhalf(mx);
    const float m_new = fmaxf(m_run, mx);
    const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
    if (__any(m_new > m_run)) {
      const float alpha = exp2f((m_run - m_use) * c);
      l_part *= alpha;
#pragma unroll
      for (int i = 0; i < NDB; ++i) oacc[i] *= alpha;
    }
    m_run = m_new;
    const float mc = -m_use * c;
    float psum = 0.f;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pv = __builtin_amdgcn_exp2f(fmaf(sa[hh][r], c, mc));
        sa[hh][r] = pv;
        psum += pv;
      }
    l_part += psum;
    u32x4_t pw[4];
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) {
      const int hh = kc >> 1, cb = (kc & 1) * 8;
      pw[kc] = u32x4_t{pack_bf2(sa[hh][cb], sa[hh][cb + 1]), pack_bf2(sa[hh][cb + 2], sa[hh][cb + 3]),
                       pack_bf2(sa[hh][cb + 4], sa[hh][cb + 5]), pack_bf2(sa[hh][cb + 6], sa[hh][cb + 7])};
    }
    pv_tile(t, pw);
  };
  // unmasked tile with a deferred running max (SPEC; see above the kernel). The caller issues the S
  // MFMAs of tile t + 1 just before, in the same basic block.
  const float spec_thr = SPEC_TAU / c;  // raw-score headroom above the reference max
  auto finish_spec = [&](int t, f32x16_t (&sa)[2]) {
    float mx = fmaxf(sa[0][0], sa[0][1]);
#pragma unroll
    for (int r = 2; r < 16; ++r) mx = fmaxf(mx, sa[0][r]);
#pragma unroll
    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sa[1][r]);
    mx = max_xhalf(mx);
    // the reference max moves only when the tile max overshoots it by SPEC_TAU (log2 units of p):
    // p <= 2^SPEC_TAU; first tile: m_run = -inf -> m_new = mx, alpha = 0
    const bool up = mx > m_run + spec_thr;
    const float m_new = up ? mx : m_run;
    const float alpha = exp2f((m_run - m_new) * c);
    const float mcs = -m_new * c;
    float psum = 0.f;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pv = __builtin_amdgcn_exp2f(fmaf(sa[hh][r], c, mcs));
        sa[hh][r] = pv;
        psum += pv;
      }
    u32x4_t pw[4];
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) {
      const int hh = kc >> 1, cb = (kc & 1) * 8;
      pw[kc] = u32x4_t{pack_bf2(sa[hh][cb], sa[hh][cb + 1]), pack_bf2(sa[hh][cb + 2], sa[hh][cb + 3]),
                       pack_bf2(sa[hh][cb + 4], sa[hh][cb + 5]), pack_bf2(sa[hh][cb + 6], sa[hh][cb + 7])};
    }
    l_part = l_part * alpha + psum;
    m_run = m_new;
    // materialise P and l here: otherwise the compiler sinks the exp / pack work past the branch
    // into the P·V block, away from the S MFMAs of t + 1 it is meant to run beside
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) asm volatile("" : "+v"(pw[kc]));
    asm volatile("" : "+v"(l_part));
    if (__any(up)) {  // rare after the first tiles: O moves to the new reference
#pragma unroll
      for (int i = 0; i < NDB; ++i) oacc[i] *= alpha;
    }
    pv_tile(t, pw);
  };

  f32x16_t SA[2], SB[2];
  auto barrier = [&]() {  // LDS reads done + every wave here (no vmcnt drain: DMA stays in flight)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  };
  if constexpr (DMA) {
    dma_tile(0, false); dma_tile(0, true); dma_tile(1, false); dma_tile(1, true); dma_tile(2, false);
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");  // K0 V0 K1 landed (V1 K2 may fly)
    barrier();
    s_tile(0, SA);
    barrier();  // every wave's S(0) reads are done before K(3) refills slot 0
  } else {
    load_tile(0);
    store_tile(0);
    if (ntiles > 1) {
      load_tile(1);
      store_tile(1);
    }
    __syncthreads();
    if (ntiles > 2) load_tile(2);
    s_tile(0, SA);
  }
  auto step = [&](int t, f32x16_t (&cur)[2], f32x16_t (&nxt)[2]) {
    if constexpr (DMA) {
      dma_tile(t + 3, false);  // slot of K(t): read by S(t) in step t - 1
      dma_tile(t + 2, true);   // slot of V(t - 1): read by P·V(t - 1) in step t - 1
    }
    const int kb = t * KT;
    const bool nx = t + 1 < ntiles && (t + 1) * KT < wave_end;
    // unmasked for every query of this wave (the smallest query sees the tile's last key)
    const bool clean = kb + KT <= Lk && (!causal || kb + KT - 1 <= P + wq0);
    if (SPEC && nx && clean) {
      s_tile(t + 1, nxt);
      finish_spec(t, cur);
    } else if (SPEC && clean && kb < wave_end) {
      finish_spec(t, cur);
    } else {
      if (nx) s_tile(t + 1, nxt);
      if (kb < wave_end) finish(t, cur);
    }
    if constexpr (DMA) {
      asm volatile("s_waitcnt vmcnt(6)" ::: "memory");  // K(t + 2), V(t + 1) landed
      barrier();
    } else {
      if (t + 2 < ntiles) store_tile(t + 2);   // its buffer (t - 1) % 3 was last read before the previous barrier
      if (t + 3 < ntiles) load_tile(t + 3);
      __syncthreads();
    }
  };
  for (int t = 0; t < ntiles; t += 2) {
    step(t, SA, SB);
    if (t + 1 < ntiles) step(t + 1, SB, SA);
  }
  if constexpr (DMA) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // trailing no-traffic pieces

  const float l_tot = sum_xhalf(l_part);
  const float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
  if (qvalid) {
    bf16_t* orow = o + (size_t)(s0 + qi) * ldo + h * D;
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d = db * 32 + 8 * g + 4 * hi;
        *(u32x2_t*)(orow + d) = u32x2_t{pack_bf2(oacc[db][4 * g] * inv, oacc[db][4 * g + 1] * inv),
                                        pack_bf2(oacc[db][4 * g + 2] * inv, oacc[db][4 * g + 3] * inv)};
      }
  }
}

// Dispatch order of the flash kernels (FaPrefix::rev, fa_block): causal longest query blocks first
// and the query blocks of one (sequence, kv head) pair on one XCD (737 -> 778 TF/s on the Phi-3 QA
// chunk, profiles/r4/flash_order/).
constexpr int kFaDispatch = 3;

// fp16 (the encoder's DTYPE=fp16): bidirectional or causal, no shared prefix, 4 waves x 32 queries
DA_EXPORT int da_flash_attn_f16(const void* q, const void* k, const void* v, int ldq, int ldk, int ldv,
                                const void* cu_seqlens, int B, int max_seqlen, int H, int Hkv, int D, int causal,
                                float scale, void* o, int ldo, void* stream) {
  if (H % Hkv || ldq % 8 || ldk % 8 || ldv % 8 || ldo % 4) return (int)hipErrorInvalidValue;
  if (B == 0 || max_seqlen == 0) return 0;
  const FaPrefix pre{nullptr, nullptr, 0, 0, kFaDispatch};
  dim3 grid((max_seqlen + 127) / 128, H, B);
  hipStream_t s = (hipStream_t)stream;
#define FA_ARGS16 (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, ldq, ldk, ldv, (const int*)cu_seqlens, H, Hkv, \
                  causal, scale * 1.4426950408889634f, (bf16_t*)o, ldo, pre
  switch (D) {
    case 64: flash_attn_v2_kernel<64, 4, 1, F16T><<<grid, 256, FA2Cfg<64, 4, 1>::SMEM, s>>>(FA_ARGS16); break;
    case 96: flash_attn_v2_kernel<96, 4, 1, F16T><<<grid, 256, FA2Cfg<96, 4, 1>::SMEM, s>>>(FA_ARGS16); break;
    default: return (int)hipErrorInvalidValue;
  }
#undef FA_ARGS16
  return (int)hipGetLastError();
}

// flash_attn_v2_kernel<D, NW, 1>: NW waves x 32 queries per workgroup (QH = 2, 64 queries per wave, is
// kept in the kernel but not instantiated: no shape runs it).
template <int D, int NW>
static int launch_fa2(const void* q, const void* k, const void* v, int ldq, int ldk, int ldv, const void* cu_seqlens,
                      int B, int max_seqlen, int H, int Hkv, int causal, float sl2e, void* o, int ldo, FaPrefix pre,
                      hipStream_t s) {
  using C = FA2Cfg<D, NW, 1>;
  if constexpr (C::SMEM > 64 * 1024) {
    static bool attr_set = false;
    if (!attr_set) {
      (void)hipFuncSetAttribute((const void*)flash_attn_v2_kernel<D, NW, 1>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                C::SMEM);
      attr_set = true;
    }
  }
  dim3 grid(pre.tail ? 1 : (max_seqlen + C::QB - 1) / C::QB, H, B);
  flash_attn_v2_kernel<D, NW, 1><<<grid, 64 * NW, C::SMEM, s>>>(
      (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, ldq, ldk, ldv, (const int*)cu_seqlens, H, Hkv, causal, sl2e,
      (bf16_t*)o, ldo, pre);
  return (int)hipGetLastError();
}

// Causal D = 96 (the Phi-3 prefill) runs the software-pipelined kernel (flash_attn_pipe: 576 -> 656
// TF/s; the short bidirectional BGE sequences, 8 tiles, lose to its longer pipeline fill, 617 -> 531
// at D = 64, profiles/r2/attn_bench_v5.txt) with the speculative softmax (654 -> 689 TF/s,
// profiles/r3/attn_bench_spec.txt) and LDS-DMA K / V tiles when the prefix is whole 64-key tiles and
// the operands 16-B aligned (711 TF/s); every other shape the 4-wave flash_attn_v2_kernel (8 waves
// at D = 128: Llama-3 prefill, profiles/r2/attn_bench_v4.txt).
template <int D, bool DMA>
static constexpr int fa_pipe_smem() {
  return 3 * ((DMA ? 64 * D * 2 : FA2Cfg<D, 4, 1>::KBUF) + FA2Cfg<D, 4, 1>::VBUF);
}

template <bool DMA>
static int launch_fa_pipe(const void* q, const void* k, const void* v, int ldq, int ldk, int ldv, const void* cu_seqlens,
                          int B, int max_seqlen, int H, int Hkv, int causal, float sl2e, void* o, int ldo,
                          FaPrefix pre, hipStream_t s) {
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)flash_attn_pipe_kernel<96, true, DMA>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, fa_pipe_smem<96, DMA>());
    attr_set = true;
  }
  dim3 grid(pre.tail ? 1 : (max_seqlen + 127) / 128, H, B);
  flash_attn_pipe_kernel<96, true, DMA><<<grid, 256, fa_pipe_smem<96, DMA>(), s>>>(
      (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, ldq, ldk, ldv, (const int*)cu_seqlens, H, Hkv, causal, sl2e,
      (bf16_t*)o, ldo, pre);
  return (int)hipGetLastError();
}

// pre_k / pre_v: shared-prefix K/V of KV head 0 in a cache slot (nullptr / pre_len 0: none),
// pre_hstride: elements between KV heads there (max_seq * D).
// kv_slot / kv_pos (nullable; per token, int32): the sequences' own keys are read from the KV cache
// k_cache / v_cache [slots, Hkv, max_seq, D] (pre_hstride = max_seq * D) instead of k / v — causal
// D = 96 only.
// tail_only: per (sequence, head) only the query block holding the sequence's last token is computed
// and stored (128 rows; 256 on the 8-wave D = 128 kernel), bit-identical to the full launch's rows;
// the other rows of o are not written. Both the pipelined and the flash_attn_v2 kernels take it.
DA_EXPORT int da_flash_attn_v2(const void* q, const void* k, const void* v, int ldq, int ldk, int ldv,
                               const void* cu_seqlens, int B, int max_seqlen, int H, int Hkv, int D, int causal,
                               float scale, void* o, int ldo, const void* pre_k, const void* pre_v,
                               long long pre_hstride, int pre_len, const void* kv_slot, const void* kv_pos,
                               const void* k_cache, const void* v_cache, int tail_only, void* stream) {
  const bool from_cache = kv_slot != nullptr;
  if (from_cache) {
    if (!causal || D != 96 || !kv_pos || !k_cache || !v_cache || pre_hstride < (long long)D ||
        pre_hstride % D || ((uintptr_t)k_cache | (uintptr_t)v_cache) % 16)
      return (int)hipErrorInvalidValue;
    k = k_cache; v = v_cache; ldk = ldv = D;  // rows D apart inside a (slot, head) block
  }
  if (H % Hkv || ldq % 8 || ldk % 8 || ldv % 8 || ldo % 4) return (int)hipErrorInvalidValue;
  if (pre_len < 0 || (pre_len > 0 && (!pre_k || !pre_v || pre_hstride < (long long)pre_len * D)))
    return (int)hipErrorInvalidValue;
  if (B == 0 || max_seqlen == 0) return 0;
  const float sl2e = scale * 1.4426950408889634f;
  hipStream_t s = (hipStream_t)stream;
  const FaPrefix pre{(const bf16_t*)pre_k, (const bf16_t*)pre_v, pre_hstride, pre_len, kFaDispatch,
                     (const int*)kv_slot, (const int*)kv_pos, (const bf16_t*)k_cache, (const bf16_t*)v_cache,
                     from_cache ? (long long)Hkv * pre_hstride : 0LL, tail_only ? 1 : 0};
  if (causal && D == 96) {
    const bool dma = pre_len % 64 == 0 && ((uintptr_t)k | (uintptr_t)v | (uintptr_t)pre_k | (uintptr_t)pre_v) % 16 == 0;
    if (dma) return launch_fa_pipe<true>(q, k, v, ldq, ldk, ldv, cu_seqlens, B, max_seqlen, H, Hkv, causal, sl2e, o, ldo, pre, s);
    return launch_fa_pipe<false>(q, k, v, ldq, ldk, ldv, cu_seqlens, B, max_seqlen, H, Hkv, causal, sl2e, o, ldo, pre, s);
  }
#define FA2(DD, NW) launch_fa2<DD, NW>(q, k, v, ldq, ldk, ldv, cu_seqlens, B, max_seqlen, H, Hkv, causal, sl2e, o, ldo, pre, s)
  switch (D) {
    case 32: return FA2(32, 4);
    case 64: return FA2(64, 4);
    case 96: return FA2(96, 4);  // bidirectional
    case 128: return FA2(128, 8);
    default: return (int)hipErrorInvalidValue;
  }
#undef FA2
}
