"""Exact-integer operands for the GEMM kernels: inputs on which ONE wrong term a[m,k] * w[n,k] moves
an output element by >= 1, and the correct output is known bit for bit. Pure torch; importable
without a GPU. The counterpart of tests/attn_probes.py.

A[m,k] is +-1 on the row's live columns and 0 elsewhere, W[n,k] is one of -2, -1, +1, +2 (never 0),
bias[n] and resid[m,n] are integers in [-8, 8]: all exact in bf16, fp16 and e4m3. Every product and
every partial sum is an integer far below 2^24, so it is exact in fp32 in ANY summation order (MFMA
order, split-K partials, gemm_dk's LDS sum, the persistent loop). The one rounding left is the final
fp32 -> bf16 / fp16 conversion, round-to-nearest-even in the kernels and in torch alike.

A case has L = ceil(K / 3072) layouts: the 64-column block j of A is live in layout j % L, so every
column is live in exactly one layout and an output has at most 3072 nonzero terms (standard
deviation <= sqrt(2.5 * 3072) ~ 88): few outputs leave |y| <= 256, where bf16 holds every integer.
One launch per layout; assert_covered() asserts that every (m, k) was live in some launch.

check() is the criterion, check_reference() the condition (on the reference alone) that keeps it
sharp: at most 1 % of a launch's outputs are not representable in the output type, and no
accumulator reaches 2^24.

W8A8 (gemm_fp8): aq = A cast to e4m3 and sa = per-row powers of two from 2^-3 .. 2^3, not quant_fp8's
amax / 448. A power-of-two scale keeps the significand, so y = sa * n is representable exactly when n
is. The residual of such a case is resid[m,n] * max(sa[m], 1) (still a small integer): with an
unscaled r in [-8, 8] and sa = 8 the sum 8 n + r needs 3 more significand bits than n, most outputs
of a K = 1024 product would be rounded and the 1 % condition could not hold."""
import torch

EPI_NONE, EPI_BIAS, EPI_GELU, EPI_SWIGLU, EPI_RESID = 0, 1, 2, 3, 4
LINEAR = (EPI_NONE, EPI_BIAS, EPI_RESID)
BLOCK = 64          # columns of A that share a layout
MAX_LIVE = 3072     # live columns of a row per launch
MAX_ROUNDED = 0.01  # share of a launch's outputs that may be unrepresentable in the output type
FP8 = torch.float8_e4m3fn
POISON = 3.0        # what the padding of a row-padded operand holds: a stray read moves the output


def n_layouts(K: int) -> int:
    return max(1, -(-K // MAX_LIVE))


def live_columns(K: int, layout: int) -> torch.Tensor:
    """bool [K]: the columns of A that are live in this layout."""
    return (torch.arange(K) // BLOCK) % n_layouts(K) == layout


def padded(t: torch.Tensor, extra: int = 16, fill: float = POISON) -> torch.Tensor:
    """A view of t's values whose rows are `extra` elements longer than its width (fill in the gap)."""
    buf = torch.full((t.shape[0], t.shape[1] + extra), fill, dtype=torch.float32, device=t.device)
    buf[:, :t.shape[1]] = t.float()
    return buf.to(t.dtype)[:, :t.shape[1]]


def neighbour(r: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    """The next representable value above (up) / below r, r in bf16 or fp16."""
    bits = r.contiguous().view(torch.int16).to(torch.int32)
    mono = torch.where(bits >= 0, bits, -(bits & 0x7FFF))  # monotonic in the value
    mono = mono + torch.where(up, 1, -1)
    back = torch.where(mono >= 0, mono, (-mono) - 0x8000)
    return back.to(torch.int16).view(r.dtype)


def rounded_mask(ref_exact: torch.Tensor, dtype=torch.bfloat16) -> torch.Tensor:
    """bool: the elements of the exact (fp64) result that the output type cannot hold."""
    return ref_exact.to(dtype).double() != ref_exact


def failures(got: torch.Tensor, ref_exact: torch.Tensor, epi: int = EPI_NONE) -> torch.Tensor:
    """bool mask of the elements of `got` (bf16 / fp16) that miss the criterion against the exact
    fp64 result. Linear epilogues: a representable element bit for bit, a rounded one either of its
    two neighbours. GELU / SwiGLU: |got - ref| <= rel |ref| + 2^-20, rel = 2^-7 (bf16) / 2^-10 (fp16):
    at least one ulp at ref; the second term covers the tails where the activation underflows."""
    dtype = got.dtype
    assert dtype in (torch.bfloat16, torch.float16) and got.shape == ref_exact.shape
    ref = ref_exact.double().to(got.device)
    g = got.double()
    if epi not in LINEAR:
        rel = 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -10
        return ~((g - ref).abs() <= rel * ref.abs() + 2.0 ** -20)
    r = ref.to(dtype)
    rd = r.double()
    other = neighbour(r, rd < ref).double()  # the representable value on the other side of ref
    ok = torch.where(rd == ref, g == ref, (g == rd) | (g == other))
    return ~ok


def check(got, ref_exact, epi: int = EPI_NONE, what: str = ""):
    bad = failures(got, ref_exact, epi)
    n = int(bad.sum())
    if n:
        i = tuple(int(x) for x in bad.nonzero()[0])
        raise AssertionError(f"{what}: {n} / {bad.numel()} elements miss the exact criterion; first at {i}: "
                             f"got {float(got[i])}, exact {float(ref_exact[i])}")


def check_reference(ref_exact, acc_max: float, dtype=torch.bfloat16, epi: int = EPI_NONE, what: str = ""):
    """The condition on the reference alone: no accumulator reaches 2^24 and, for a linear epilogue,
    at most MAX_ROUNDED of the outputs are not representable in the output type."""
    assert acc_max < 2 ** 24, f"{what}: an accumulator may reach {acc_max} >= 2^24"
    assert bool(torch.isfinite(ref_exact).all()), f"{what}: the reference is not finite"
    if epi in LINEAR:
        share = rounded_mask(ref_exact, dtype).double().mean().item()
        assert share <= MAX_ROUNDED, f"{what}: {share:.4%} of the outputs are rounded (> {MAX_ROUNDED:.0%})"


def rotate_90(x: torch.Tensor, cs: torch.Tensor) -> torch.Tensor:
    """x [T, heads, D] (fp64) with pairs (2i, 2i+1) turned by cs [T, D/2, 2] (attn_probes.rope_table_90)."""
    x1, x2 = x[..., 0::2], x[..., 1::2]
    c, s = cs[:, None, :, 0].double(), cs[:, None, :, 1].double()
    return torch.stack([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).flatten(-2)


class GemmCase:
    """Operands and exact results of one [M, K] x [N, K]^T product, seeded; everything on the CPU.

    w (fp32 values of W), bias [N], resid [M, N]; a(l) is layout l's activation operand; exact(l, epi)
    the fp64 result of the epilogue on the exact integer product. fp8_act: the W8A8 form (sa, and the
    residual scaled as the module text says). SwiGLU reads W as 16-row gate / up groups interleaved
    (ops/reference.py interleave_gate_up) and has N / 2 outputs."""

    def __init__(self, M: int, N: int, K: int, seed: int = 0, fp8_act: bool = False):
        self.M, self.N, self.K, self.L = M, N, K, n_layouts(K)
        g = torch.Generator().manual_seed(seed * 1000003 + M * 7919 + N * 104729 + K)
        self._a = (torch.randint(0, 2, (M, K), generator=g) * 2 - 1).double()
        mag = torch.randint(1, 3, (N, K), generator=g)
        self.w = ((torch.randint(0, 2, (N, K), generator=g) * 2 - 1) * mag).float()
        self.bias = torch.randint(-8, 9, (N,), generator=g).float()
        self.resid = torch.randint(-8, 9, (M, N), generator=g).float()
        self.sa = None
        if fp8_act:
            self.sa = torch.exp2(torch.randint(-3, 4, (M,), generator=g).float())
            self.resid = self.resid * self.sa.clamp_min(1.0)[:, None]
        self._seen = torch.zeros(M, K, dtype=torch.bool)
        self._pre = {}

    def a(self, l: int) -> torch.Tensor:
        """fp32 [M, K]: layout l's A (marks its live columns as launched)."""
        live = live_columns(self.K, l)
        self._seen[:, live] = True
        return (self._a * live.double()[None]).float()

    def assert_covered(self):
        missing = int((~self._seen).sum())
        assert missing == 0, f"{missing} of {self._seen.numel()} (m, k) were live in no launch"

    def acc_max(self, l: int, code_max: float = 2.0) -> float:
        """The largest magnitude any partial sum of layout l can reach (code_max: the weight operand's
        largest magnitude as the MFMA sees it: 2 for bf16 / fp16, the e4m3 code for an fp8 copy)."""
        return float(live_columns(self.K, l).sum()) * code_max

    def pre(self, l: int) -> torch.Tensor:
        """fp64 [M, N]: the exact product (times sa for a W8A8 case), before any epilogue."""
        if l not in self._pre:
            live = live_columns(self.K, l)
            y = (self._a * live.double()[None]) @ self.w.double().t()  # integers < 2^53: exact in fp64
            self._pre[l] = y if self.sa is None else y * self.sa.double()[:, None]
        return self._pre[l]

    def exact(self, l: int, epi: int = EPI_NONE, bias: bool = None) -> torch.Tensor:
        """fp64: the epilogue in fp64 on the exact product. bias: add the bias (default: BIAS only)."""
        y = self.pre(l)
        if (epi == EPI_BIAS) if bias is None else bias:
            y = y + self.bias.double()
        if epi == EPI_RESID:
            y = y + self.resid.double()
        elif epi == EPI_GELU:
            y = torch.nn.functional.gelu(y)
        elif epi == EPI_SWIGLU:
            yy = y.view(self.M, self.N // 32, 2, 16)
            y = (torch.nn.functional.silu(yy[:, :, 0]) * yy[:, :, 1]).reshape(self.M, self.N // 2)
        return y

    def w8(self):
        """(codes e4m3 [N, K], scale fp32 [N]) of W with power-of-two row scales; asserts the copy is W."""
        from docagents_amd.ops import reference as R
        q, s = R.quant_weight_fp8_pow2(self.w.to(torch.bfloat16))
        assert torch.equal(q.float() * s[:, None], self.w), "the fp8 weight copy is not W exactly"
        assert bool((torch.log2(s) == torch.log2(s).round()).all())
        return q, s

    def code_max(self) -> float:
        q, _ = self.w8()
        return float(q.float().abs().max())


def rope_exact(case: GemmCase, l: int, pos, slot, cos_sin, H: int, Hkv: int, D: int, k_cache, v_cache):
    """gemm_rope's exact results: qkv fp64 [M, N] with the q / k heads turned by cos_sin[pos], and the
    caches (fp64 copies of k_cache / v_cache [slots, Hkv, max_seq, D]) with row (slot, pos) written."""
    qkv = case.pre(l).view(case.M, H + 2 * Hkv, D).clone()
    qkv[:, :H + Hkv] = rotate_90(qkv[:, :H + Hkv], cos_sin[pos.long()])
    kc, vc = k_cache.double().clone(), v_cache.double().clone()
    kc[slot.long(), :, pos.long()] = qkv[:, H:H + Hkv]
    vc[slot.long(), :, pos.long()] = qkv[:, H + Hkv:]
    return qkv.reshape(case.M, -1), kc, vc

