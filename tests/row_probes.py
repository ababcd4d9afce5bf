"""Inputs on which ONE wrong element of a row kernel moves the output, for the norms, embeddings,
pooling, row quantisation and the stand-alone RoPE kernels (ops/csrc/norm.hip, rope_cache_kernel,
rope_cache_kv8): builders, fp64 references and criteria. Pure torch; importable without a GPU. The
counterpart of tests/attn_probes.py and tests/gemm_probes.py, whose failures / neighbour / padded /
POISON / rotate_90 / rope_table_90 are used here, not copied.

Every kernel of norm.hip gives thread t the 8-element chunks t + i * blockDim, i < MAXCH, and then
reduces over the wave and the block (or, in the many-row forms, over one wave). Two row kinds:

SPIKE rows test the reductions. A width D has nch = D / 8 chunks and nch spike rows; row r is zero
except at column 8 r + (r % 8), where it holds +-2^k (k = r % 7, the sign alternates). Every chunk,
and every element slot of a chunk, carries the whole sum of some row: a dropped spike turns
inv = (x^2 / D + eps)^-0.5 into eps^-0.5 (a factor of ~300 at D = 16384, more below), a doubled one
changes it by sqrt(2).

DENSE rows test the mapping of x, the weight and the output. x[j] is one of +-0.5, +-1, +-2 (seeded),
so every square is a multiple of 0.25 and a row's sum of squares (< 2^24 quarters) is exact in fp32
in ANY order. The weight w[j] = 1 + 4 L(j) / 128, L(j) in 0..31, is a bf16 value in [1, 2) (ulp
2^-7) with the CONDITION that w[j] differs from w[j +- 1], w[j +- 8], w[j +- 512] and w[j +- 2048]
(the neighbouring element, chunk, wave and loop pass of a 256-thread workgroup) by >= 4 ulps: a
weight taken from any of those moves the output by >= 2^-6 of its value, two bf16 ulps or more.
separated() asserts the condition on the inputs. The bias is the same construction scaled into
[1/8, 1/4) with alternating sign. Residual form: resid[m, j] is an integer in [-8, 8] and
x = h - resid, all multiples of 0.5 below 128 and therefore exact in bf16, as is their fp32 sum h: the
updated residual stream is compared with torch.equal.

RMSNorm criterion (gemm_probes.failures, linear form: a representable output bit for bit, otherwise
either bf16 neighbour of the fp64 value). The kernel's fp32 value: ss is exact; ss / D, + eps, the
hardware rsqrt (1 ulp = 2^-23), and the two products v * inv * w are five roundings, and eps itself
is the fp32 image of the double (2^-25 of at most the whole sum). inv carries half of the first two
and the eps term plus the rsqrt: together < 2^-21 of the value, against half a bf16 ulp of >= 2^-9.
So the fp32 value rounds to the exact value where bf16 holds it and to one of its two neighbours
where not; nothing else can occur, and nothing in the bound depends on the sum's length.

LayerNorm criterion: |got - ref| <= rel (|t| + |b|) + 2^-20, t = (x - mean) inv g, rel = 2^-7 (bf16)
or 2^-10 (fp16). One output ulp is at most rel |t + b| and the rounding itself half of that; the
kernel's fp32 error is far smaller: the row sums are exact (multiples of 0.5), mean is one rounding,
and the variance sum of D terms (<= 64 serial per thread, 6 wave steps, <= 4 waves) carries < 80
roundings, < 2^-17.6 of var and half that of inv. The constant 2^-20 covers fp16 subnormals. It still
bites: the bias of a neighbouring chunk is >= 2^-6 |b| away, a spike dropped from the mean moves the
zero columns by g / sqrt(D) >= 2^-7 against a bound of 2^-7 (2^-7 g + 1/4). Dense rows are conditioned
on |mean| <= 0.25 so that x - mean never cancels; constant rows (variance 0) must give b.

Fused fp8 output of LayerNorm / embeddings + LayerNorm (layernorm_kernel quantises the fp32 row it
holds in registers, not the bf16 row it stored): scale within F32_REL = 2^-16 of amax |ref| / 448
(the fp32 bound above, rounded up), and each code the nearest e4m3 value of ref / scale with the
kernel's own scale; the value across the nearest tie is accepted only where the quotient lies within
F32_REL (|t| + |b|) / scale + 2^-20 |q| of that tie, about one element in 2^11.

rmsnorm_q8 quantises the bf16-rounded row: its scale is amax / 448 of that bf16 row bit for bit and
a code may cross a tie only within 2^-20 |q| (x * (1 / scale) against x / scale: two roundings).

pool_l2norm: every token of a sequence of length L has 1 in column 0 and one token t* holds L in
column 8 c + (c % 8) (column 1 for chunk 0, where column 0 is taken). The mean is (1, 1) in the two
columns whatever fp32 1 / L is, since both are the same product; the unit vector is 1 / sqrt(2) in
both and exact zeros elsewhere. The kernel's roundings (1 / L, two products, the hardware rsqrt) stay
below 2^-22 of a value <= 1: fp32 outputs within 2^-21, bf16 outputs by the neighbour rule. A dropped
or doubled token changes the ratio of the two columns by >= 1 / 300 = 2^-8.2.

quant_fp8 rows: row r is 2^e (e cycling over -6..4) times e4m3 values, +-448 2^e at the spike column
and all other finite e4m3 codes of both signs elsewhere. amax / 448 = 2^e, 1 / 2^e and every quotient
are exact: scale and code bytes bit for bit.

RoPE: integer rows in [-8, 8] without zeros and with x1 != +-x2 in every pair, turned by
rope_table_90 (pair i at position p by 90 p (i + 1) degrees) at positions that are no multiple of 4,
so that neighbouring pairs and neighbouring positions turn differently: the result is a signed
permutation, exact in bf16, compared with torch.equal. Integers up to 8 times a power of two are
e4m3 values, so the fp8 cache's codes and power-of-two scales are exact too."""
import functools

import torch

import gemm_probes as G
from attn_probes import rope_table_90  # noqa: F401  (re-exported for the test files)
from gemm_probes import POISON, failures, neighbour, padded, rotate_90  # noqa: F401

BF16, F16, FP8 = torch.bfloat16, torch.float16, torch.float8_e4m3fn
MAXCH = 8
MAX_D = MAXCH * 256 * 8
# one-workgroup-per-row widths: two chunks; a partly idle single wave; a second wave with two live
# lanes; a second loop pass with two live lanes; half the threads with two chunks; a last pass short
# by two chunks; all eight passes full
WIDTHS = (16, 272, 528, 2064, 3072, 16368, 16384)
ROWS_WIDTHS = (2048, 3072, 4096)   # the one-wave-per-row kernels (route_m >= 1024)
F16_WIDTHS = (272, 1024, 16384)
EMBED_WIDTHS = (16, 1024, 3072, 4096, 16384)
N_DENSE = 3
RMS_EPS, LN_EPS = 1e-5, 1e-12
F32_REL = 2.0 ** -16               # bound on the fp32 error of a LayerNorm output, see the module text
NEIGHBOUR_OFFSETS = (1, 8, 64 * 8, 256 * 8)
DENSE_VALUES = torch.tensor([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], dtype=torch.float64)
POOL_LENGTHS = (1, 2, 63, 64, 65, 300)


def row_threads(D: int) -> int:
    return min(256, max(64, (D // 8 + 63) // 64 * 64))


def spike_col(r: int) -> int:
    return 8 * r + (r % 8)


def spike_cols(n: int) -> torch.Tensor:
    r = torch.arange(n)
    return 8 * r + r % 8


def spike_values(n: int) -> torch.Tensor:
    r = torch.arange(n)
    return torch.exp2((r % 7).double()) * (1 - 2 * (r % 2)).double()


def spike_rows(D: int) -> torch.Tensor:
    """fp64 [D / 8, D]: row r holds +-2^(r % 7) at column 8 r + (r % 8) and zeros elsewhere."""
    n = D // 8
    x = torch.zeros(n, D, dtype=torch.float64)
    x[torch.arange(n), spike_cols(n)] = spike_values(n)
    return x


def dense_rows(D: int, n: int = N_DENSE, seed: int = 0) -> torch.Tensor:
    """fp64 [n, D] of +-0.5, +-1, +-2, seeded, each row conditioned on |mean| <= 0.25."""
    g = torch.Generator().manual_seed(seed * 7919 + D)
    rows = []
    while len(rows) < n:
        row = DENSE_VALUES[torch.randint(0, 6, (D,), generator=g)]
        if abs(float(row.mean())) <= 0.25:
            rows.append(row)
    return torch.stack(rows)


def _level(D: int) -> torch.Tensor:
    j = torch.arange(D)
    return (5 * j + 3 * (j // 8) + 7 * (j // 512) + 11 * (j // 2048)) % 32


def weight(D: int) -> torch.Tensor:
    """fp64 [D]: 1 + 4 L(j) / 128 in [1, 2); exact in bf16 and fp16."""
    return 1.0 + 4.0 * _level(D).double() / 128.0


def bias(D: int) -> torch.Tensor:
    """fp64 [D]: +-(1 + 4 L'(j) / 128) / 8, L' = (3 L + 5) % 32, the sign alternating per chunk."""
    lv = (3 * _level(D) + 5) % 32
    sign = (1 - 2 * ((torch.arange(D) // 8) % 2)).double()
    return sign * (1.0 + 4.0 * lv.double() / 128.0) / 8.0


def separated(w: torch.Tensor, ulp: float, what: str = "w"):
    """The weight condition: w[j] and w[j + o] differ by >= 4 ulps for o in NEIGHBOUR_OFFSETS."""
    assert bool((w.to(BF16).double() == w).all()), f"{what} is not exact in bf16"
    for o in NEIGHBOUR_OFFSETS:
        if o < w.numel():
            gap = float((w[o:] - w[:-o]).abs().min())
            assert gap >= 4 * ulp, f"{what}[j] and {what}[j + {o}] differ by {gap / ulp} ulps (< 4)"


def exact_in(t: torch.Tensor, dtype) -> bool:
    return bool((t.to(dtype).double() == t).all())


def small_ints(shape, seed: int, lo: int = -8, hi: int = 8) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).double()


# ------------------------------------------------------------------------------------------ RMSNorm
class RmsCase:
    """M = D / 8 spike rows + N_DENSE dense rows h [M, D] (fp64), the weight w, and for the residual
    form resid (integers) with x = h - resid. ref: the fp64 RMSNorm of h."""

    def __init__(self, D: int, eps: float = RMS_EPS):
        self.D, self.eps = D, eps
        self.h = torch.cat([spike_rows(D), dense_rows(D)])
        self.M = self.h.shape[0]
        self.w = weight(D)
        self.resid = small_ints((self.M, D), seed=D + 1).float()
        inv = 1.0 / torch.sqrt((self.h ** 2).mean(1, keepdim=True) + eps)
        self.ref = self.h * inv * self.w

    @property
    def x_resid(self):
        return self.h - self.resid

    def check_reference(self):
        what = f"rmsnorm D={self.D}"
        assert bool(torch.isfinite(self.ref).all()), f"{what}: the reference is not finite"
        assert bool(((self.h * 2).round() == self.h * 2).all()), f"{what}: rows are not multiples of 0.5"
        quarters = float((self.h ** 2).sum(1).max()) * 4
        assert quarters < 2 ** 24, f"{what}: a sum of squares reaches {quarters} quarters >= 2^24"
        separated(self.w, 2.0 ** -7)
        for t in (self.h, self.resid, self.x_resid):
            assert exact_in(t, BF16), f"{what}: an operand is not exact in bf16"
        n = self.D // 8
        assert bool(((self.h[:n] != 0).sum(1) == 1).all()) and bool((self.h[:n] != 0).any(0).view(n, 8).any(1).all())
        zeros = self.h[:n] == 0
        assert bool((self.ref[:n][zeros] == 0).all())


def check_rms(got: torch.Tensor, case: RmsCase, what: str = ""):
    """gemm_probes' linear criterion; the zeros of the spike rows by value (the kernel may write -0)."""
    G.check(got, case.ref, G.EPI_NONE, what)


# ---------------------------------------------------------------------------------------- LayerNorm
CONSTANTS = (3.0, -0.5, 0.0)


class LnCase:
    """Spike rows, dense rows and constant rows h [M, D]; gain g, bias b; t = (h - mean) inv g and
    ref = t + b in fp64. resid / x_resid as in RmsCase."""

    def __init__(self, D: int, eps: float = LN_EPS):
        self.D, self.eps = D, eps
        const = torch.tensor(CONSTANTS, dtype=torch.float64)[:, None].expand(-1, D)
        self.h = torch.cat([spike_rows(D), dense_rows(D), const])
        self.M = self.h.shape[0]
        self.n_const = len(CONSTANTS)
        self.g, self.b = weight(D), bias(D)
        self.resid = small_ints((self.M, D), seed=D + 2).float()
        mean = self.h.mean(1, keepdim=True)
        var = ((self.h - mean) ** 2).mean(1, keepdim=True)
        self.t = (self.h - mean) / torch.sqrt(var + eps) * self.g
        self.ref = self.t + self.b

    @property
    def x_resid(self):
        return self.h - self.resid

    def check_reference(self):
        what = f"layernorm D={self.D}"
        assert bool(torch.isfinite(self.ref).all()), f"{what}: the reference is not finite"
        assert bool(((self.h * 2).round() == self.h * 2).all())
        assert float(self.h.abs().sum(1).max()) * 2 < 2 ** 24, f"{what}: a row sum is not exact in fp32"
        n = self.D // 8
        dense = self.h[n:n + N_DENSE]
        assert float(dense.mean(1).abs().max()) <= 0.25, f"{what}: a dense row has |mean| > 0.25"
        separated(self.g, 2.0 ** -7, "g")
        separated(self.b, 2.0 ** -10, "b")
        for dt in (BF16, F16):
            for t in (self.h, self.resid, self.x_resid, self.g, self.b):
                assert exact_in(t, dt), f"{what}: an operand is not exact in {dt}"
        const = slice(self.M - self.n_const, self.M)
        assert bool((self.t[const] == 0).all()) and bool((self.ref[const] == self.b).all())


def ln_bound(t: torch.Tensor, b: torch.Tensor, dtype) -> torch.Tensor:
    rel = 2.0 ** -7 if dtype == BF16 else 2.0 ** -10
    return rel * (t.abs() + b.abs()) + 2.0 ** -20


def ln_failures(got: torch.Tensor, t: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """bool mask of the elements of got (bf16 / fp16) outside |got - (t + b)| <= rel (|t| + |b|) + 2^-20."""
    assert got.dtype in (BF16, F16) and got.shape == t.shape
    t, b = t.to(got.device), b.to(got.device)
    g = got.double()
    return ~((g - (t + b)).abs() <= ln_bound(t, b, got.dtype)) | ~torch.isfinite(g)


def check_ln(got, t, b, what: str = ""):
    bad = ln_failures(got, t, b)
    n = int(bad.sum())
    if n:
        i = tuple(int(x) for x in bad.nonzero()[0])
        raise AssertionError(f"{what}: {n} / {bad.numel()} elements miss the LayerNorm bound; first at {i}: "
                             f"got {float(got[i])}, exact {float((t + b.to(t.device))[i])}")


class EmbedLnCase:
    """LnCase's rows as sums word[ids] + pos[positions] + type[types]: pos (5 rows) and type (2 rows)
    hold small integers, type[1] != type[0] in every column, and word[ids[i]] = h[i] - pos - type, all
    exact in bf16 / fp16 and in the kernel's fp32 sum. ids is a reversal (first and last table row
    included), positions cycles over every pos row, types holds both values. types=None: word_none,
    the table for which type[0] completes every row."""

    def __init__(self, ln: LnCase):
        self.ln = ln
        M, D = ln.M, ln.D
        self.pos = small_ints((5, D), seed=D + 3, lo=-2, hi=2)
        t0 = small_ints((1, D), seed=D + 4, lo=-1, hi=1)
        self.type = torch.cat([t0, t0 + 1 + small_ints((1, D), seed=D + 5, lo=0, hi=1)])
        self.ids = torch.arange(M - 1, -1, -1, dtype=torch.int32)
        self.positions = (torch.arange(M) % 5).to(torch.int32)
        self.types = ((torch.arange(M) // 2) % 2).to(torch.int32)
        rest = ln.h - self.pos[self.positions.long()]
        self.word = torch.empty(M, D)
        self.word[self.ids.long()] = (rest - self.type[self.types.long()]).float()
        self.word_none = torch.empty(M, D)
        self.word_none[self.ids.long()] = (rest - self.type[0]).float()

    def check_reference(self):
        assert int(self.ids.min()) == 0 and int(self.ids.max()) == self.word.shape[0] - 1
        assert set(self.types.tolist()) == {0, 1} and set(self.positions.tolist()) == set(range(5))
        assert bool((self.type[0] != self.type[1]).all())
        for dt in (BF16, F16):
            for t in (self.word, self.word_none, self.pos, self.type):
                assert exact_in(t.double(), dt)
        s = self.word[self.ids.long()].float() + self.pos[self.positions.long()].float()
        assert torch.equal((s + self.type[self.types.long()].float()).double(), self.ln.h)


# ------------------------------------------------------------------------------------------- e4m3
def e4m3_other(ref: torch.Tensor, q: torch.Tensor) -> torch.Tensor:
    """The e4m3 value (fp64) on the other side of q from ref = the e4m3 rounding of q (saturating)."""
    byte = ref.contiguous().view(torch.uint8).to(torch.int32)
    mag = byte & 0x7F
    away = q.abs() > ref.double().abs()
    mag = (mag + torch.where(away, 1, -1)).clamp(0, 0x7E)
    out = (mag | torch.where(q < 0, 0x80, 0)).to(torch.uint8).view(FP8)
    return out.double()


def fp8_failures(codes: torch.Tensor, q: torch.Tensor, slack: torch.Tensor) -> torch.Tensor:
    """bool mask of the codes (e4m3) that are neither the e4m3 rounding of the exact quotient q (fp64)
    nor, where q lies within slack of the tie between them, the value across that tie. By value."""
    ref = q.clamp(-448, 448).float().to(FP8)
    rd = ref.double()
    other = e4m3_other(ref, q)
    near = (q.clamp(-448, 448) - (rd + other) / 2).abs() <= slack
    got = codes.view(FP8).double() if codes.dtype == torch.uint8 else codes.double()
    return ~((got == rd) | (near & (got == other)))


def quant_rule_failures(codes, scale, y16: torch.Tensor):
    """rmsnorm_q8's contract on a bf16 row y16 it never stores: scale = amax / 448 in fp32 bit for
    bit (all-zero row: 1), codes = e4m3(y16 / scale), a tie crossed only within 2^-20 |q|.
    Returns (rows with a wrong scale, wrong codes), both bool masks."""
    amax = y16.double().abs().amax(1)
    # the fp32 quotient through fp64 (a tensor / scalar division may multiply by a rounded 1 / 448)
    want = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax)).float()
    q = y16.double() / want.double()[:, None]
    return scale[:y16.shape[0]] != want, fp8_failures(codes, q, 2.0 ** -20 * q.abs())


def fused_fp8_failures(codes, scale, t: torch.Tensor, b: torch.Tensor):
    """The fused fp8 output of LayerNorm against the fp64 row ref = t + b, see the module text.
    Returns (rows with a wrong scale, wrong codes), both bool masks."""
    t, b = t.to(codes.device), b.to(codes.device)
    ref = t + b
    amax = ref.abs().amax(1)
    want = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    s = scale[:ref.shape[0]].double()
    bad_scale = ~((s - want).abs() <= F32_REL * want)
    q = ref / s[:, None]
    slack = F32_REL * (t.abs() + b.abs()) / s[:, None] + 2.0 ** -20 * q.abs()
    return bad_scale, fp8_failures(codes, q, slack)


E4M3_CODES = torch.cat([torch.arange(0x00, 0x7F), torch.arange(0x81, 0xFF)]).to(torch.uint8)  # finite, no -0


class QuantCase:
    """quant_fp8 rows [D / 8, D]: x = 2^e(r) * e4m3 values (fp64, exact in bf16); codes (uint8) and
    scale = 2^e(r) are the expected outputs, bit for bit."""

    def __init__(self, D: int):
        self.D = D
        n = D // 8
        r = torch.arange(n)
        self.e = (r % 11) - 6
        idx = (torch.arange(D)[None, :] * 5 + r[:, None] * 3) % E4M3_CODES.numel()
        codes = E4M3_CODES[idx]
        top = torch.where(r % 2 == 0, 0x7E, 0xFE).to(torch.uint8)
        # no second +-448 in a row: the maximum lives in the spike chunk alone
        codes = torch.where((codes & 0x7F) == 0x7E, codes - 1, codes)
        codes[r, spike_cols(n)] = top
        self.codes = codes
        self.scale = torch.exp2(self.e.float())
        self.x = codes.view(FP8).double() * self.scale.double()[:, None]

    def check_reference(self):
        assert exact_in(self.x, BF16) and bool(torch.isfinite(self.x).all())
        n = self.D // 8
        amax = self.x.abs().amax(1)
        assert torch.equal(amax, 448.0 * self.scale.double())
        assert bool(((self.x.abs() == amax[:, None]).sum(1) == 1).all())
        assert torch.equal(self.x.abs().argmax(1), spike_cols(n))
        if self.D >= 2048:  # 5 j + 3 r runs over all 254 codes within a row
            assert set(self.codes.unique().tolist()) == set(E4M3_CODES.tolist())


# -------------------------------------------------------------------------------------------- pool
def pool_spike_col(c: int) -> int:
    return 8 * c + (c % 8) if c else 1


class PoolCase:
    """Sequences for pool_l2norm at width D, see the module text. The first 15 are POOL_LENGTHS x
    (t* first / middle / last) on the LAST chunks of the row, then come an empty sequence, an
    all-zero sequence, and sequences of length 1 and 2 for every remaining chunk. h fp64 [T, D], cu
    int32 [B + 1]; ref(mode): fp64 [B, D]. kinds[b]: 'probe', 'empty' or 'zero'."""

    def __init__(self, D: int):
        self.D = D
        nch = D // 8
        plan = []
        for L in POOL_LENGTHS:
            for ts in sorted({0, L // 2, L - 1}):
                plan.append((L, ts))
        seqs, c = [], nch - 1
        for L, ts in plan:
            seqs.append(("probe", L, ts, c % nch))
            c -= 1
        seqs.insert(7, ("empty", 0, 0, 0))
        seqs.insert(11, ("zero", 5, 0, 0))
        i = 0
        while c >= 0:
            L = 1 + i % 2
            seqs.append(("probe", L, i % L, c))
            c -= 1
            i += 1
        T = sum(s[1] for s in seqs)
        self.h = torch.zeros(T, D)
        cu, self.kinds, self.cols = [0], [], []
        for kind, L, ts, c in seqs:
            s0 = cu[-1]
            if kind == "probe":
                self.h[s0:s0 + L, 0] = 1.0
                self.h[s0 + ts, pool_spike_col(c)] = float(L)
            cu.append(s0 + L)
            self.kinds.append(kind)
            self.cols.append(pool_spike_col(c))
        self.cu = torch.tensor(cu, dtype=torch.int32)
        self.B = len(seqs)
        self.chunks = {c for kind, _, _, c in seqs if kind == "probe"} | {0}

    def ref(self, mode: int, device="cpu") -> torch.Tensor:
        """fp64 [B, D]: the first token (mode 0, or an empty sequence: the row at s0) or the mean of
        the sequence's tokens, divided by its norm; a zero vector stays zero."""
        h = self.h.to(device).double()
        cu = self.cu.to(device).long()
        lens = cu[1:] - cu[:-1]
        v = h[cu[:-1]]
        if mode == 1:
            seg = torch.repeat_interleave(torch.arange(self.B, device=device), lens)
            sums = torch.zeros(self.B, self.D, dtype=torch.float64, device=device).index_add_(0, seg, h)
            v = torch.where((lens > 0)[:, None], sums / lens.clamp_min(1)[:, None], v)
        n = v.norm(dim=1, keepdim=True)
        return torch.where(n > 0, v / n.clamp_min(1e-300), v)

    def check_reference(self):
        assert exact_in(self.h.double(), BF16) and exact_in(self.h.double(), F16)
        assert self.chunks == set(range(self.D // 8)), "a chunk carries no sequence's spike"
        assert int(self.cu[-1]) == self.h.shape[0] and "empty" in self.kinds and "zero" in self.kinds
        assert self.cu.tolist()[self.kinds.index("empty") + 1] < self.h.shape[0]  # the row at s0 exists
        ref = self.ref(1)
        for b, kind in enumerate(self.kinds):
            if kind == "probe":
                want = torch.zeros(self.D, dtype=torch.float64)
                want[0] = want[self.cols[b]] = 0.5 ** 0.5
                assert float((ref[b] - want).abs().max()) < 1e-15
            elif kind == "zero":
                assert bool((ref[b] == 0).all())
        assert bool(torch.isfinite(self.ref(0)).all())


def pool_failures32(got: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    ref = ref.to(got.device)
    return ~((got.double() - ref).abs() <= 2.0 ** -21) | ((ref == 0) & (got != 0))


# -------------------------------------------------------------------------------------------- embed
def embed_table(D: int, rows: int = 23) -> torch.Tensor:
    """fp64 [rows, D]: distinct dense rows (every pair differs in about 5 / 6 of the columns)."""
    t = dense_rows(D, rows, seed=11)
    assert all(not torch.equal(t[i], t[j]) for i in range(rows) for j in range(i))
    return t


def embed_ids(rows: int = 23, T: int = 37) -> torch.Tensor:
    """T ids with 0, the last row and repeats."""
    ids = (torch.arange(T) * 7 + 3) % rows
    ids[0], ids[1], ids[T - 1], ids[T - 2] = 0, rows - 1, rows - 1, 0
    return ids.to(torch.int32)


# --------------------------------------------------------------------------------------------- RoPE
ROPE_SHAPES = ((32, 8, 128), (32, 32, 96), (8, 1, 64), (4, 4, 96))  # the first two exceed 256 work items
ROPE_T, ROPE_MAX_SEQ, ROPE_SLOTS = 21, 64, 3
CACHE_FILL = 7.0


class RopeCase:
    """qkv [T, (H + 2 Hkv) D] of integers in [-8, 8], no zero, x1 != +-x2 in every pair; T distinct
    (slot, pos) with pos % 4 != 0 including 1 and max_seq - 1; cs = rope_table_90(max_seq, D).
    exact(rotate_q) -> (qkv, k rows, v rows) in fp64; caches(...) the expected [slots, Hkv, max_seq, D]."""

    def __init__(self, H: int, Hkv: int, D: int, T: int = ROPE_T, max_seq: int = ROPE_MAX_SEQ):
        self.H, self.Hkv, self.D, self.T, self.max_seq = H, Hkv, D, T, max_seq
        g = torch.Generator().manual_seed(H * 131 + Hkv * 17 + D)
        n = T * (H + 2 * Hkv) * D // 2
        m1 = torch.randint(1, 9, (n,), generator=g)
        m2 = 1 + (m1 - 1 + torch.randint(1, 8, (n,), generator=g)) % 8  # another magnitude in 1..8
        s = torch.randint(0, 2, (2, n), generator=g) * 2 - 1
        self.qkv = torch.stack([m1 * s[0], m2 * s[1]], dim=-1).double().view(T, (H + 2 * Hkv) * D)
        ok = [p for p in range(1, max_seq) if p % 4]
        order = [1, max_seq - 1] + [p for p in ok if p not in (1, max_seq - 1)][::2]
        self.pos = torch.tensor(order[:T], dtype=torch.int32)
        self.slot = (torch.arange(T) % ROPE_SLOTS).to(torch.int32)
        self.cs = rope_table_90(max_seq, D)

    def check_reference(self):
        x = self.qkv.view(self.T, -1, 2)
        assert bool((x != 0).all()) and float(x.abs().max()) <= 8 and bool((x[..., 0].abs() != x[..., 1].abs()).all())
        p = self.pos.tolist()
        assert all(q % 4 for q in p) and 1 in p and self.max_seq - 1 in p and {q % 4 for q in p} == {1, 2, 3}
        assert len(set(zip(self.slot.tolist(), p))) == self.T and max(p) < self.max_seq
        items = (self.H + 2 * self.Hkv) * (self.D // 8)
        assert exact_in(self.exact(True)[0], BF16)
        return items

    def exact(self, rotate_q: bool = True):
        H, Hkv, D = self.H, self.Hkv, self.D
        x = self.qkv.view(self.T, H + 2 * Hkv, D).clone()
        lo = 0 if rotate_q else H
        x[:, lo:H + Hkv] = rotate_90(x[:, lo:H + Hkv], self.cs[self.pos.long()])
        return x.reshape(self.T, -1), x[:, H:H + Hkv].clone(), x[:, H + Hkv:].clone()

    def caches(self, rotate_q: bool = True, fill: float = CACHE_FILL):
        _, k, v = self.exact(rotate_q)
        kc = torch.full((ROPE_SLOTS, self.Hkv, self.max_seq, self.D), fill, dtype=torch.float64)
        vc = kc.clone()
        kc[self.slot.long(), :, self.pos.long()] = k
        vc[self.slot.long(), :, self.pos.long()] = v
        return kc, vc


@functools.lru_cache(maxsize=1)
def rms_case(D: int) -> RmsCase:
    return RmsCase(D)


@functools.lru_cache(maxsize=1)
def ln_case(D: int) -> LnCase:
    return LnCase(D)
