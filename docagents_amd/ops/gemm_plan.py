"""The routing table of every ``[M, K] x [N, K]^T`` product: which entry point of the kernel
library runs it, on which tile, with how many K splits and how much fp32 workspace.

Pure Python (no torch, no ctypes): ``kernels.gemm`` / ``gemm_dk`` / ``gemm_resid_norm`` launch
what ``plan`` / ``plan_dk`` / ``plan_resid_norm`` return, the decoder calls the op ``weight_op``
names and keeps the fp8 weight copies ``keeps_w8_copy`` asks for, and ``ops/reference.py`` (the CPU
decoder) re-exports these objects: nothing else decides. ``tests/test_gemm_plan_cpu.py`` pins the
tables against ``tests/golden/gemm_routes.json`` and ``tests/golden/w8_routes.json``.

Tile ids (the ABI of ``da_gemm_bf16``'s ``switch``, csrc/gemm.hip): big tiles when the grid fills
the CUs, skinny tiles (+ split-K) for decode-sized M.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

EPI_NONE, EPI_BIAS, EPI_GELU, EPI_SWIGLU, EPI_RESID = 0, 1, 2, 3, 4

TILE_128x128 = 1      # 128x128, 2x2 waves
TILE_64x128 = 2       # 64x128 weight-streaming decode tile, 4 k-tiles in flight
TILE_32x128 = 3       # 32x128 weight-streaming decode tile, 4 k-tiles in flight
TILE_8P_256 = 7       # 256x256 phase-split (gemm8p); 4 is an accepted alias
TILE_GEMV = 6         # GEMV (M = 1), can fuse the input RMSNorm
TILE_128x128_PF4 = 8  # 128x128, 4 k-tiles in flight (mid-M weight streaming)
TILE_128x64_PF4 = 9   # 128x64, 4 k-tiles in flight: one tile per 64 weight rows
TILE_8P_128 = 10      # 128x256 phase-split (gemm8p)
TILE_DK = 12          # the gemm_dk hand-off (da_gemm_dk / da_gemm_dk_splitk); Python-side, da_gemm_bf16 rejects it
TILE_4W = 13          # 256x256 four-wave (gemm4w)

_FAMILY = {TILE_GEMV: "gemv", 4: "gemm8p", TILE_8P_256: "gemm8p", TILE_8P_128: "gemm8p", TILE_4W: "gemm4w"}

# Decode GEMMs with 2..64 rows: gemm_dk (csrc/gemm_dk.hip: K split across the 4 waves of a
# workgroup and summed through LDS, no split-K partials, no reduce launch). False: the 64x128 /
# 32x128 tiles + split-K + reduce (bench/ab_arms.py DA_DECODE_DK=0). plan()'s cache is keyed on it.
DECODE_DK = True
# 33..64 rows keep the gemm_dk layer structure (norms deferred into the consumer) on the split-K
# tiles: the narrow dk tiles re-read the activation block once per 16-64 weight rows there
# (bench/midm_chain.py, profiles/r3/dk/), so gemm_dk() routes those rows to da_gemm_dk_splitk
# (reduce + residual + row sums of squares; the consumer's reduce applies the row scale)
DK_MAX_M = 64
DK_SPLITK_ABOVE = 32
PREFILL_M = 640  # rows from which a product runs on the phase-split kernel, unsplit
WIDE_N = 8192    # 65..128 rows: weight rows from which the 64x128 tile runs unsplit (see _auto_tile)


class GemmPlan(NamedTuple):
    family: str    # "gemv" | "dk" | "dk_splitk" | "dk_w8" | "tile" | "gemm8p" | "gemm4w"
    tile: int
    splits: int
    ws_bytes: int  # fp32 split-K partials: splits * M * N * 4, 0 where the launch needs no workspace


def gemv_fusable(M: int, N: int, K: int, epi: int = EPI_NONE) -> bool:
    """True when gemm() runs the batch-1 GEMV (which can also fuse the input RMSNorm)."""
    return M == 1 and K % 512 == 0 and N % 4 == 0 and (epi != EPI_SWIGLU or N % 32 == 0)


def _decode_epi(N: int, epi: int) -> bool:
    return epi in (EPI_NONE, EPI_BIAS, EPI_RESID, EPI_SWIGLU) and (epi != EPI_SWIGLU or N % 32 == 0)


def _gemv_w8_shape(N: int, K: int, epi: int) -> bool:
    return K % 1024 == 0 and N % 4 == 0 and _decode_epi(N, epi)


def gemv_w8_fusable(M: int, N: int, K: int, epi: int = EPI_NONE) -> bool:
    """True when gemm_w8() accepts the product: the batch-1 GEMV on fp8 weights (csrc/gemv_w8.hip)."""
    return M == 1 and _gemv_w8_shape(N, K, epi)


def gemv_w4_fusable(M: int, N: int, K: int, epi: int = EPI_NONE) -> bool:
    """True when gemm_w4() accepts the product: the batch-1 GEMV on MXFP4 weights (csrc/gemv_w4.hip),
    every shape of the fp8 GEMV's rule (a k-block is 1024 elements there too). No shape is held back:
    on the five Phi-3-mini products the launch took 0.46-0.69x the bf16 GEMV's time (O projection
    3.95 vs 5.75 us, the closest), the two runs differing by at most 3 % (profiles/w4/README.md)."""
    return M == 1 and _gemv_w8_shape(N, K, epi)


def keeps_w4_copy(N: int, K: int, epi: int = EPI_NONE) -> bool:
    """True when a decoder with MXFP4 weights keeps the codes and scales of the [N, K] product: only
    the one-row GEMV streams them (0.53125 B per weight kept, on top of the bf16 tensor)."""
    return gemv_w4_fusable(1, N, K, epi)


def _dk_shape(N: int, K: int, epi: int) -> bool:
    return K % 256 == 0 and N % 16 == 0 and _decode_epi(N, epi)  # gemm_dk and gemm_dk_w8 alike


def dk_fusable(M: int, N: int, K: int, epi: int = EPI_NONE) -> bool:
    """True when gemm() runs a decode-sized product on gemm_dk (no split-K)."""
    return DECODE_DK and 2 <= M <= DK_MAX_M and _dk_shape(N, K, epi)


def _mid_rows(M: int) -> bool:
    return 64 < M <= 128  # a batch-128 decode step


def _auto_tile(M: int, N: int, K: int, splits: int, cus: int) -> int:
    """The tile of a product whose caller named none; splits == 0: the split count is chosen too.

    Decode-sized M: 32x128 tiles up to 32 rows, 64x128 to 64; 65..128 rows (a batch-128 decode
    step): N >= 8192 (QKV, gate/up, LM head: >= 128 weight tiles) the 64x128 tile over the two row
    blocks without split-K, else one 128x64 weight-streaming tile per 64 weight rows with split-K
    (profiles/r5/midm/decode_gemm_sweep_m128.txt, weights cold: QKV 28.0 vs 33.5 us, gate/up 30.5 vs
    47.4 us at 128 rows vs the 128x64 tile at split 4; O / down best on the 128x64 tile at split 4);
    129..639 rows the 64x128 tile over ceil(M/64) row blocks; from 640 rows the phase-split kernel
    with the row-tile height of fewer workgroup waves (prefill_bm; 32-layer Phi-3 chain and
    single-GEMM sweeps: bench/midm_chain.py, bench/gemm_ab.py, profiles/r2, r3). A caller's own
    split count (> 1) always runs on the 64x128 tile above 32 rows."""
    if M <= 32:
        return TILE_32x128
    if splits == 0 and _mid_rows(M) and N < WIDE_N:
        return TILE_128x64_PF4
    if M < PREFILL_M or splits > 1:
        return TILE_64x128
    if K < 128:
        return TILE_128x128
    return TILE_8P_256 if prefill_bm(M, N, cus) == 256 else TILE_8P_128


def prefill_bm(M: int, N: int, cus: int) -> int:
    """Row-tile height for a non-RoPE prefill product: the one with fewer workgroup WAVES over the
    chip's CUs, weighting a 128-row tile's time as 0.72 of a 256-row one (measured at M = 2930:
    128-row tiles took 0.61-0.73 of the 256-row tile time, profiles/r3/gemm_ab_batch1_prefill_tiles.txt).
    At M ~ 2.6k (the batch-1 prefill of the p50 path) the O / down projections (N = 3072) then run
    252 128-row tiles in one wave instead of 132 256-row tiles on half the chip; QA-sized chunks
    (M ~ 64k) keep 256 (the round-3 rule, 256 rows once the 256-row grid reached half the chip,
    measured 65.5 vs 74.9 us per O projection at M ~ 2.6k: profiles/r4/bm_rule/)."""
    ntn = -(-N // 256)
    w256, w128 = -(-(-(-M // 256) * ntn) // cus), -(-(-(-M // 128) * ntn) // cus)
    return 128 if w128 * 72 < w256 * 100 else 256


def auto_splits(M: int, N: int, K: int) -> int:
    """Split-K for decode-sized M: the largest power of two keeping <= 256 workgroups (one per CU)
    and >= 4 K-steps per split. With 4 k-tiles in flight per workgroup (gemm.hip PF) a tile needs
    fewer splits to cover HBM latency, and fewer splits = fewer partial bytes to reduce. From a
    graph-replayed sweep with weights streamed cold from HBM, as in a real decode step
    (profiles/decode_gemm_prefetch_sweep_r1.jsonl: matches the best split on 17 of 20 Phi-3 /
    Llama-3-8B shapes at M = 16 / 64, within 0.7 us on the rest)."""
    if M >= PREFILL_M:
        return 1
    ksteps = K // 64
    if _mid_rows(M):  # (see _auto_tile) wide N: no split; else 4 splits, fewer if K is short
        if N >= WIDE_N:
            return 1
        s = 4
        while s > 1 and (ksteps % s or ksteps // s < 4):
            s //= 2
        return s
    tiles = -(-M // (32 if _auto_tile(M, N, K, 0, 0) == TILE_32x128 else 64)) * -(-N // 128)
    # 65..639 rows run the 64x128 tile over ceil(M/64) row blocks (the row blocks of one weight tile
    # share it through L2): up to 4 workgroups per CU below 256 rows, 2.5 from 256 (32-layer Phi-3
    # chain, bench/midm_chain.py, profiles/r2/midm_chain.txt: split 4 best at M = 65 / 128, 2 at 192 /
    # 256, 1 from 384)
    cap = 256 if M <= 64 else (1024 if M < 256 else 640)
    s = 1
    while tiles * s * 2 <= cap and ksteps % (s * 2) == 0 and ksteps // (s * 2) >= 4:
        s *= 2
    return s


def dk_splits(N: int, K: int) -> int:
    """Split-K of the 33..64-row route (64x128 tiles): the largest of 2, 3, 4, 6, 8, 12, 16 that keeps
    the grid within one round of 256 workgroups and >= 4 K-steps of 64 per split; at least 2 (the
    reduce carries the epilogue). 3 is the point of this list: the Phi-3 QKV projection (72 tiles)
    18.7 us at 3 splits vs 21.8 at 2 and 25.7 at 4 (bench/splitk_m64.py, profiles/r3/splitk_m64.txt)."""
    tiles, ks = (N + 127) // 128, K // 64
    best = 2
    for s in (2, 3, 4, 6, 8, 12, 16):
        if ks % s == 0 and ks // s >= 4 and tiles * s <= 256:
            best = s
    return best if ks % best == 0 else 2


def _dk_splitk_parts(M: int, N: int) -> bool:
    return DK_SPLITK_ABOVE < M <= DK_MAX_M and N % 512 == 0  # the reduce writes one ssq part per 512 columns


def dk_parts(N: int, M: int = 0) -> int:
    """Row-norm partial sums an EPI_RESID gemm_dk of width N and M rows writes (the consumer's part
    count): one per dk output tile (csrc/gemm_dk.hip dk_bn; da_gemm_dk_parts reports the same), or
    one per 512 columns on the 33..64-row split-K route."""
    if _dk_splitk_parts(M, N):
        return N // 512
    bn = 64 if N // 64 >= 192 else 32 if N // 32 >= 192 else 16
    return -(-N // bn)


def plan_dk(M: int, N: int, K: int, ssq_out: bool = False) -> GemmPlan:
    """gemm_dk()'s launch: da_gemm_dk, or above DK_SPLITK_ABOVE rows da_gemm_dk_splitk unless an
    ssq_out needs the dk kernel's own part layout (N % 512 != 0)."""
    if _dk_splitk_parts(M, N) or (DK_SPLITK_ABOVE < M <= DK_MAX_M and not ssq_out):
        splits = dk_splits(N, K)
        return GemmPlan("dk_splitk", TILE_DK, splits, splits * M * N * 4)
    return GemmPlan("dk", TILE_DK, 1, 0)


# gemm_dk on the decoder's e4m3 weight copy (csrc/gemm_dk_w8.hip): 2..32 rows only; 33..128 rows
# stream the copy on the split-K tiles (tile_w8_fusable below)
DK_W8_MAX_M = 32


def dk_w8_fusable(M: int, N: int, K: int, epi: int = EPI_NONE) -> bool:
    """True when a decode step runs the product on gemm_dk_w8 (fp8 weights) instead of gemm_dk: every
    shape the kernel takes at 2..32 rows (one row is the fp8 GEMV's, gemv_w8_fusable). fp8 beat the
    bf16 gemm_dk on all five Phi-3-mini products at 4, 16 and 32 rows (0.67-0.91x, profiles/w8dk/README.md),
    so no shape is held back. An EPI_RESID launch tiles like gemm_dk and writes dk_parts(N) parts."""
    return 2 <= M <= DK_W8_MAX_M and _dk_shape(N, K, epi)


def plan_dk_w8(M: int, N: int, K: int, ssq_out: bool = False) -> GemmPlan:
    """gemm_dk_w8()'s launch: always da_gemm_dk_w8, one launch, no split-K, no workspace."""
    return GemmPlan("dk_w8", TILE_DK, 1, 0)


# The 64x128 / 128x64 weight-streaming tiles on the decoder's e4m3 weight copy (csrc/gemm_tile_w8.hip):
# the 33..128-row decode steps, between gemm_dk_w8's rows and the prefill's
TILE_W8_ABOVE = DK_W8_MAX_M
TILE_W8_MAX_M = 128
TILE_W8_SHORT_K_ROWS = 96  # 65..96 rows: products with K <= 3072 on the 128x64 tile stay on bf16 (tile_w8_fusable)


def _tile_w8_shape(N: int, K: int, epi: int) -> bool:
    return K >= 128 and K % 64 == 0 and N >= 8 and N % 8 == 0 and _decode_epi(N, epi)


def tile_w8_fusable(M: int, N: int, K: int, epi: int = EPI_NONE) -> bool:
    """True when a decode step of M rows runs the product on the fp8 tile kernels (gemm_tile_w8,
    gemm_dk_splitk_w8, gemm_resid_norm_w8) instead of the bf16 ones: every shape the kernels take at
    33..128 rows. Which op runs it is the decoder body's choice; each launches the tile, split count
    and workspace of the bf16 plan for the same (M, N, K, epi) (plan_tile_w8 / plan_dk_splitk_w8 /
    plan_resid_norm_w8), so the step keeps its bits. Measurements: profiles/w8mid/README.md.

    Held back:
    * K = 64. The kernels take a single k-tile (and are tested on it), but such a product has no weight
      stream to halve, and a decoder that narrow keeps no fp8 copy at all.
    * 65..TILE_W8_SHORT_K_ROWS rows on the 128x64 tile (N < WIDE_N) with K <= 3072: Phi-3-mini's O
      projection (3072 x 3072) at 96 rows ran 17.04 us against 16.95 us on bf16 (1.006x; the repeated
      bf16 arm differed by 0.1 %), the one loss among the 20 (product, row count) pairs measured; it won
      at 128 rows (0.984x) and the down projection (K = 8192) was level at 96 (0.999x). The 128x64 tile
      re-reads the whole activation block per 64 weight rows, so there the weight bytes are not the bound."""
    if _mid_rows(M) and M <= TILE_W8_SHORT_K_ROWS and N < WIDE_N and K <= 3072:
        return False
    return TILE_W8_ABOVE < M <= TILE_W8_MAX_M and _tile_w8_shape(N, K, epi)


def _w8_tile(p: GemmPlan, what: str) -> GemmPlan:
    if p.tile not in (TILE_64x128, TILE_128x64_PF4):
        raise ValueError(f"{what}: the bf16 plan's tile {p.tile} has no fp8 form (tiles 2 and 9 only)")
    return p


def plan_tile_w8(M: int, N: int, K: int, epi: int = EPI_NONE, *, cus: int) -> GemmPlan:
    """gemm_tile_w8()'s launch: what plan() gives gemm() for the same product. Where that is the
    33..64-row split-K hand-off (plan_dk -> da_gemm_dk_splitk without norm or row sums) it is the
    same launch by its tile name: 64x128 partials at dk_splits + gemm_splitk_reduce."""
    p = plan(M, N, K, epi, cus=cus)
    if p.family == "dk_splitk":
        p = GemmPlan("tile", TILE_64x128, p.splits, p.ws_bytes)
    return _w8_tile(p, "gemm_tile_w8")


def plan_dk_splitk_w8(M: int, N: int, K: int, ssq_out: bool = False) -> GemmPlan:
    """gemm_dk_splitk_w8()'s launch: plan_dk's split-K route (33..64 rows; an ssq_out needs
    N % 512 == 0, the reduce's part layout). ValueError where plan_dk runs the dk kernel itself."""
    p = plan_dk(M, N, K, ssq_out)
    if p.family != "dk_splitk":
        raise ValueError(f"gemm_dk_splitk_w8: M={M} N={N} ssq_out={ssq_out} is not on the split-K route")
    return p


def plan_resid_norm_w8(M: int, N: int, K: int) -> GemmPlan:
    """gemm_resid_norm_w8()'s launch: plan_resid_norm's (tile 2 at 33..64 rows, tile 9 above)."""
    return _w8_tile(plan_resid_norm(M, N, K), "gemm_resid_norm_w8")


# Prefill products on the fp8 256x256 tile (csrc/gemm256.hip, da_gemm_fp8; LLM_PREFILL_DTYPE=fp8):
# e4m3 activations quantised per token row x the decoder's e4m3 weight copy. Rows up to 128 are a
# decode step's and keep the routes above.
PREFILL_W8_ABOVE = 128


def _prefill_w8_shape(N: int, K: int, epi: int) -> bool:
    return K % 128 == 0 and N % 8 == 0 and epi != EPI_BIAS and _decode_epi(N, epi)


def prefill_w8_fusable(M: int, N: int, K: int, epi: int = EPI_NONE) -> bool:
    """True when an fp8 prefill (prefill_dtype="fp8") runs the product of an M-row pass on
    da_gemm_fp8 instead of gemm(): every shape the kernel takes above the decode range. The rows a
    last-layer tail keeps follow the route of the M-row pass they belong to (the caller asks with
    that M), so a kept row ends with the bits the full pass gives it: the tile is fixed, there is no
    split-K and the scales are per row, so a row's result does not depend on M. Which shapes were
    measured against the bf16 route and which are taken on the rule alone: profiles/prefill8/README.md.

    Held back, from that A/B: an EPI_RESID product (its input needs a quantisation pass of its own;
    rmsnorm_q8 replaces a norm pass that runs anyway) from PREFILL_M rows whose 256x256 tiles do not
    fill the 256 CUs once and whose K is at most 3072. There the tile's K loop is too short for the
    fp8 MFMA rate to pay for the pass: Phi-3's O projection in a batch-1 prefill (M = 2930, 144 tiles)
    ran 55.8 us against 55.2 us on the bf16 route; the down projection (same tiles, K = 8192) won."""
    if not (M > PREFILL_W8_ABOVE and _prefill_w8_shape(N, K, epi)):
        return False
    underfilled = -(-M // 256) * -(-N // 256) < 256
    return not (epi == EPI_RESID and M >= PREFILL_M and underfilled and K <= 3072)


_BF16_BODY_OP = {"gemm": "gemm", "dk": "gemm_dk", "resid_norm": "gemm_resid_norm"}


@functools.lru_cache(maxsize=4096)
def weight_op(body: str, M: int, N: int, K: int, epi: int = EPI_NONE, *, ssq_out: bool = False,
              weight_dtype: str = "fp8") -> str:
    """The name of the op a decoder calls for an M-row product on a weight that has an fp8 copy (the
    bf16 op's name where the product stays on the bf16 tensor). ``body`` is the layer structure asking:

    "gemm"        the plain / GEMV body, the fused-norm body's QKV, gate/up and LM head, the MLP and the
                  logits: gemm_w8 at one row, gemm_tile_w8 at 33..128 rows, else gemm. One entry serves
                  the one-row body and the fused-norm body: their fp8 row ranges are disjoint (1 against
                  33..128), and a one-row step never takes the fused-norm body.
    "dk"          the gemm_dk body: gemm_dk_w8 at 2..32 rows, gemm_dk_splitk_w8 where plan_dk puts the
                  product on the split-K route (33..64 rows; with ssq_out only at N % 512 == 0, else the
                  dk kernel writes the parts and gemm_dk_splitk_w8 would refuse), else gemm_dk.
    "resid_norm"  the fused-norm body's O and down projections: gemm_resid_norm_w8 or gemm_resid_norm.

    The W8A8 prefill is no entry here: it swaps the activation operand too (prefill_w8_fusable).

    weight_dtype="mxfp4" (the weight has an MXFP4 copy instead): gemm_w4 for the "gemm" body at one row
    where gemv_w4_fusable holds; everything else is the body's bf16 op on the dequantised tensor."""
    if weight_dtype == "mxfp4":
        if body not in _BF16_BODY_OP:
            raise ValueError(f"weight_op: unknown body {body!r}")
        return "gemm_w4" if body == "gemm" and gemv_w4_fusable(M, N, K, epi) else _BF16_BODY_OP[body]
    if weight_dtype != "fp8":
        raise ValueError(f"weight_op: unknown weight_dtype {weight_dtype!r}")
    if body == "gemm":
        if gemv_w8_fusable(M, N, K, epi):
            return "gemm_w8"
        return "gemm_tile_w8" if tile_w8_fusable(M, N, K, epi) else "gemm"
    if body == "dk":
        if dk_w8_fusable(M, N, K, epi):
            return "gemm_dk_w8"
        on_splitk = tile_w8_fusable(M, N, K, epi) and plan_dk(M, N, K, ssq_out).family == "dk_splitk"
        return "gemm_dk_splitk_w8" if on_splitk else "gemm_dk"
    if body == "resid_norm":
        return "gemm_resid_norm_w8" if tile_w8_fusable(M, N, K, EPI_RESID) else "gemm_resid_norm"
    raise ValueError(f"weight_op: unknown body {body!r}")


def keeps_w8_copy(N: int, K: int, epi: int = EPI_NONE, *, prefill_fp8: bool = False) -> bool:
    """True when some row count sends the [N, K] product to an op that streams the fp8 copy: the
    shape conditions of gemv_w8_fusable (1 row), dk_w8_fusable (2..32), tile_w8_fusable (33..128) and,
    for a decoder with an fp8 prefill, prefill_w8_fusable (above 128). What tile_w8_fusable and
    prefill_w8_fusable hold back covers part of their row ranges only (65..96 rows; from PREFILL_M
    rows while the tiles underfill the chip), so a shape they take is taken at some row count."""
    return (_gemv_w8_shape(N, K, epi) or _dk_shape(N, K, epi) or _tile_w8_shape(N, K, epi)
            or (prefill_fp8 and _prefill_w8_shape(N, K, epi)))


def plan_resid_norm(M: int, N: int, K: int, tile: int = 0, splits: int = 0) -> GemmPlan:
    """gemm_resid_norm()'s launch (M <= 128): the fused reduce + norm always reads fp32 partials, so
    the workspace is needed at one split too; above 64 rows it takes the 128x64 tile only."""
    tile = tile or (TILE_128x64_PF4 if _mid_rows(M) else _auto_tile(M, N, K, 0, 0))
    if splits <= 0:
        splits = auto_splits(M, N, K)
    return GemmPlan("tile", tile, splits, splits * M * N * 4)


def plan(M: int, N: int, K: int, epi: int = EPI_NONE, *, cus: int, tile: int = 0, splits: int = 0,
         rms: bool = False, ssq_out: bool = False) -> GemmPlan:
    """gemm()'s launch. tile = 0 / splits <= 0: chosen here (both: the dk hand-off for 2..64 rows, the
    GEMV at one row, the decode tiles + auto_splits below PREFILL_M rows, the phase-split kernel
    from there); tile = TILE_DK forces gemm_dk where dk_fusable holds; an explicit tile gets a
    chosen split count only on the decode tiles. rms: the fused input RMSNorm, GEMV only.
    ValueError for a shape gemm() does not take."""
    return _plan(M, N, K, epi, cus, tile, splits, rms, ssq_out, DECODE_DK)


@functools.lru_cache(maxsize=4096)
def _plan(M, N, K, epi, cus, tile, splits, rms, ssq_out, decode_dk) -> GemmPlan:
    if K % 64 or N % 8 or (epi == EPI_SWIGLU and N % 32):
        raise ValueError(f"gemm needs K % 64 == 0 and N % 8 == 0 (SwiGLU: N % 32 == 0), got N={N} K={K}")
    auto = tile == 0 and splits <= 0
    if (tile == TILE_DK or auto) and not rms and dk_fusable(M, N, K, epi):
        return plan_dk(M, N, K, ssq_out)
    if auto and gemv_fusable(M, N, K, epi):
        tile, splits = TILE_GEMV, 1  # batch-1 decode: weight-streaming GEMV, one launch, no split-K workspace
    if rms and tile != TILE_GEMV:
        raise ValueError("fused RMSNorm needs the M == 1 GEMV path")
    if splits <= 0:
        if tile == 0:
            tile = _auto_tile(M, N, K, 0, cus)
            splits = auto_splits(M, N, K)
        elif tile in (TILE_64x128, TILE_32x128) or (tile == TILE_128x64_PF4 and M <= 128):
            splits = auto_splits(M, N, K)
        else:
            splits = 1
    elif tile == 0:
        tile = _auto_tile(M, N, K, splits, cus)
    return GemmPlan(_FAMILY.get(tile, "tile"), tile, splits, splits * M * N * 4 if splits > 1 else 0)
