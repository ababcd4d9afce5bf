"""The exact-integer GEMM criterion of tests/gemm_probes.py bites: a plain torch GEMM with the kernels'
structure (K cut into 64-wide tiles of eight 8-chunks, `splits` slices with fp32 partials, one
rounding) passes it, and each of eight one-element mutants of that GEMM fails it. No GPU needed.

The negative control runs mutants (a)-(d) under the old criterion (_close(atol=0.03, rtol=0.02) on
test_gemm's Gaussian operands): see test_old_criterion_on_gaussian_operands for what it showed."""
import pytest
import torch

import gemm_probes as G
from gemm_probes import EPI_BIAS, EPI_GELU, EPI_NONE, EPI_RESID, EPI_SWIGLU, GemmCase

# every K the GPU file launches (tests/test_gemm_probes_gpu.py); 4608 has 2 layouts, 8192 has 3
GPU_KS = [64, 128, 192, 256, 320, 384, 512, 640, 768, 1024, 1536, 3072, 4608, 8192]


def structured_gemm(a, w, splits=1, mutant=None, at=None):
    """fp32 [M, N] = a [M, K] @ w [N, K]^T summed as the kernels do: per split an fp32 partial over
    its 64-wide tiles, each tile eight 8-chunks; the partials summed in fp32. mutant / at: see MUTANTS."""
    M, K = a.shape
    N = w.shape[0]
    nk = K // 64
    assert K % 64 == 0 and nk % splits == 0
    per = nk // splits
    m0, k0, n0 = at if at is not None else (0, 0, 0)
    parts = []
    for s in range(splits):
        acc = torch.zeros(M, N)
        for t in range(s * per, (s + 1) * per):
            for c in range(8):
                lo = t * 64 + c * 8
                aa, ww = a[:, lo:lo + 8].clone(), w[:, lo:lo + 8].clone()
                hit = lo <= k0 < lo + 8
                if mutant == "skip_k" and hit:
                    aa[m0, k0 - lo] = 0
                if mutant == "double_k" and hit:
                    aa[m0, k0 - lo] *= 2
                if mutant == "swap_w_in_chunk" and hit:  # two k's of W swapped for one 16-column block
                    i, j = k0 - lo, (k0 - lo + 1) % 8
                    ww[n0:n0 + 16, [i, j]] = ww[n0:n0 + 16, [j, i]]
                if mutant == "drop_last_chunk" and lo == K - 8:
                    continue
                acc += aa @ ww.t()
        if mutant == "bf16_partial" and s == splits - 1:
            acc = acc.to(torch.bfloat16).float()
        parts.append(acc)
    y = torch.stack(parts).sum(0)
    if mutant == "swap_rows":
        y[[m0, m0 + 1]] = y[[m0 + 1, m0]]
    return y


def epilogue(y, case, epi, mutant=None, at=None, dtype=torch.bfloat16):
    """The kernels' epilogue in fp32 on the fp32 sum, rounded once."""
    if epi == EPI_BIAS:
        y = y + case.bias
    if epi == EPI_RESID:
        y = y + case.resid
    elif epi == EPI_GELU:
        y = torch.nn.functional.gelu(y)
    elif epi == EPI_SWIGLU:
        yy = y.view(y.shape[0], case.N // 32, 2, 16).clone()
        if mutant == "swap_gate_up":  # one column pair: gate read where up belongs and back
            j, c = at[2] // 32, at[2] % 16
            yy[:, j, :, c] = yy[:, j, :, c].flip(1)
        y = (torch.nn.functional.silu(yy[:, :, 0]) * yy[:, :, 1]).reshape(y.shape[0], case.N // 2)
    return y.to(dtype)


def _at(case):
    """A fixed (row, k, column) away from every edge."""
    return case.M // 3, (case.K // 2) | 5, (case.N // 2) // 32 * 32


@pytest.mark.parametrize("Kd", GPU_KS)
def test_unmutated_passes_at_every_k_and_layout(Kd):
    """The structured GEMM meets the criterion, every (m, k) is live in one launch, and the reference
    keeps its condition (<= 1 % rounded, accumulators < 2^24) at 64 x 512 outputs."""
    case = GemmCase(64, 512, Kd, seed=1)
    splits = next(s for s in (4, 3, 2, 1) if (Kd // 64) % s == 0)
    for l in range(case.L):
        a = case.a(l)
        assert int((a != 0).sum(1).max()) <= G.MAX_LIVE
        y = structured_gemm(a, case.w, splits)
        for epi in (EPI_NONE, EPI_BIAS, EPI_RESID, EPI_GELU, EPI_SWIGLU):
            ref = case.exact(l, epi)
            G.check_reference(ref, case.acc_max(l), epi=epi, what=f"K={Kd} layout {l} epi {epi}")
            G.check(epilogue(y, case, epi), ref, epi, what=f"K={Kd} layout {l} epi {epi}")
        G.check(epilogue(y, case, EPI_RESID, dtype=torch.float16), case.exact(l, EPI_RESID), EPI_RESID)
    case.assert_covered()
    assert case.code_max() * G.MAX_LIVE < 2 ** 24  # the fp8 copy's integer codes stay exact too


def test_assert_covered_sees_a_missing_layout():
    case = GemmCase(4, 16, 8192)
    case.a(0), case.a(2)
    with pytest.raises(AssertionError, match="live in no launch"):
        case.assert_covered()


def test_check_reference_refuses_a_blunt_case():
    """Outputs of ~ +-3000 are mostly unrepresentable in bf16: the condition, not the kernel, fails."""
    ref = (torch.arange(4096, dtype=torch.float64) - 2048).view(64, 64) * 3 + 1
    with pytest.raises(AssertionError, match="rounded"):
        G.check_reference(ref, 1000.0)
    with pytest.raises(AssertionError, match="2\\^24"):
        G.check_reference(torch.zeros(2, 2, dtype=torch.float64), 2.0 ** 24)


def test_rounded_element_takes_either_neighbour_only():
    ref = torch.tensor([[257.0, 255.0, -513.0, 1025.0]], dtype=torch.float64)  # bf16 ulp: 2, 1, 4, 8
    for got, bad in (([256.0, 255.0, -512.0, 1024.0], 0), ([258.0, 255.0, -516.0, 1032.0], 0),
                     ([260.0, 255.0, -512.0, 1024.0], 1), ([256.0, 254.0, -512.0, 1024.0], 1),
                     ([256.0, 255.0, -508.0, 1024.0], 1), ([256.0, 255.0, -512.0, 1016.0], 1)):
        assert int(G.failures(torch.tensor([got]).to(torch.bfloat16), ref).sum()) == bad, got
    ref16 = torch.tensor([[2049.0, 2047.0]], dtype=torch.float64)  # fp16 ulp: 2, 1
    assert int(G.failures(torch.tensor([[2048.0, 2047.0]]).half(), ref16).sum()) == 0
    assert int(G.failures(torch.tensor([[2052.0, 2046.0]]).half(), ref16).sum()) == 2


# mutant -> the epilogue it is run under
MUTANTS = {"skip_k": EPI_NONE, "double_k": EPI_BIAS, "swap_w_in_chunk": EPI_NONE, "drop_last_chunk": EPI_RESID,
           "swap_rows": EPI_NONE, "swap_gate_up": EPI_SWIGLU}
SHAPES = [(64, 384, 256, 1), (40, 416, 768, 3), (64, 512, 3072, 4), (33, 512, 8192, 2)]


@pytest.mark.parametrize("mutant", MUTANTS)
@pytest.mark.parametrize("M,N,Kd,splits", SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}s{s[3]}" for s in SHAPES])
def test_mutant_fails_the_exact_criterion(mutant, M, N, Kd, splits):
    """(a) one k of one row skipped, (b) one k counted twice, (c) two k's of W swapped inside one
    8-chunk for one 16-column block, (d) the last 8-chunk of the last split dropped, (f) two output
    rows swapped, (g) SwiGLU gate and up swapped for one column pair: each fails check(); the
    unmutated GEMM passes on the same operands."""
    case = GemmCase(M, N, Kd, seed=2)
    epi = MUTANTS[mutant]
    at = _at(case)
    l = int((at[1] // G.BLOCK) % case.L)                     # the layout in which column k is live
    if mutant == "drop_last_chunk":
        l = int(((Kd - 8) // G.BLOCK) % case.L)
    a, ref = case.a(l), case.exact(l, epi)
    G.check_reference(ref, case.acc_max(l), epi=epi)
    G.check(epilogue(structured_gemm(a, case.w, splits), case, epi), ref, epi)
    bad = epilogue(structured_gemm(a, case.w, splits, mutant, at), case, epi, mutant, at)
    assert int(G.failures(bad, ref, epi).sum()) > 0, f"{mutant} passes the exact criterion"


def test_bf16_partial_fails_the_exact_criterion():
    """(e) one split's partial rounded to bf16 before the reduce. Visible only where a PARTIAL leaves
    |y| <= 256: at K = 3072 in two splits (1536 terms, sigma ~ 62) a few of 128 x 2048 partials do.
    With four splits of 768 terms (sigma ~ 44) none does: such a launch cannot show this mutant, on
    these operands or any other whose partial sums bf16 holds."""
    case = GemmCase(128, 2048, 3072, seed=3)
    a, ref = case.a(0), case.exact(0)
    G.check_reference(ref, case.acc_max(0))
    G.check(structured_gemm(a, case.w, 2).to(torch.bfloat16), ref)
    bad = structured_gemm(a, case.w, 2, "bf16_partial").to(torch.bfloat16)
    assert int(G.failures(bad, ref).sum()) > 0


def test_fp8_code_exponent_mutant_fails():
    """(h) one e4m3 code's exponent off by one (bit 3 of the code byte): the weight doubles."""
    case = GemmCase(17, 48, 768, seed=4)
    q, s = case.w8()
    m0, k0, n0 = _at(case)
    a, ref = case.a(0), case.exact(0)
    G.check(structured_gemm(a, q.float() * s[:, None]).to(torch.bfloat16), ref)
    codes = q.view(torch.uint8).clone()
    codes[n0, k0] ^= 8
    w_bad = codes.view(G.FP8).float() * s[:, None]
    assert float((w_bad - case.w).abs().sum()) in (0.5, 1.0, 2.0)  # one weight halved or doubled
    bad = structured_gemm(a, w_bad).to(torch.bfloat16)
    assert int(G.failures(bad, ref).sum()) == case.M  # column n0 of every row (every a[m, k0] is +-1)


def test_w8a8_case_is_exact_with_power_of_two_row_scales():
    case = GemmCase(40, 64, 1024, seed=5, fp8_act=True)
    aq = case.a(0).to(G.FP8)
    assert torch.equal(aq.float(), case.a(0)) and bool(((case.sa >= 0.125) & (case.sa <= 8)).all())
    q, s = case.w8()
    acc = structured_gemm(aq.float(), q.float())              # integer codes: exact in fp32
    assert float(acc.abs().max()) < 2 ** 24
    for epi in (EPI_NONE, EPI_RESID):
        ref = case.exact(0, epi)
        G.check_reference(ref, case.acc_max(0, case.code_max()), epi=epi)
        y = acc * case.sa[:, None] * s[None, :] + (case.resid if epi == EPI_RESID else 0)
        G.check(y.to(torch.bfloat16), ref, epi)


def _old_close_mismatches(got, ref, atol=0.03, rtol=0.02):
    got, ref = got.float(), ref.float()
    return int(((got - ref).abs() > atol + rtol * ref.abs()).sum())


OLD_SEES = {}  # filled below: (shape, mutant) -> mismatches under the old criterion


@pytest.mark.parametrize("M,N,Kd", [(64, 384, 256), (512, 768, 3072)])
def test_old_criterion_on_gaussian_operands(M, N, Kd):
    """Negative control: test_gemm's operands (a ~ N(0, 1), w ~ N(0, 1/K), bf16) and its criterion
    _close(atol=0.03, rtol=0.02) against the fp32 reference, under mutants (a)-(d).

    What it showed, as (outputs flagged by the old criterion, outputs the mutant moved); the operands
    are seeded, so the outcome is asserted:
                          (a) skip   (b) double   (c) swap in chunk   (d) drop last chunk
      (64, 384, 256)      296 / 377  296 / 380    550 / 1004          18906 / 24301
      (512, 768, 3072)      0 / 651    0 / 647   1074 / 6321         140873 / 378119
    Only (a) and (b) at K = 3072 PASS the old criterion: one term is ~ K^-0.5 = 0.018, below the
    tolerance. The others do NOT pass there, so they are not forced: at K = 256 one term is ~ 0.06,
    above atol, and (c) / (d) move 16 M / M N outputs by several terms, of which the old criterion
    flags the 17-78 % where the move exceeds 0.03 + 0.02 |ref|. It sees such a mistake through the
    tail of the operand distribution, in a share of the moved outputs that falls as K grows; on the
    probe operands every moved output fails (the tests above)."""
    g = torch.Generator().manual_seed(M * 1000 + N)
    a = torch.randn(M, Kd, generator=g).to(torch.bfloat16).float()
    w = (torch.randn(N, Kd, generator=g) * Kd ** -0.5).to(torch.bfloat16).float()
    ref = (a @ w.t()).to(torch.bfloat16)
    at = (M // 3, (Kd // 2) | 5, (N // 2) // 32 * 32)
    assert _old_close_mismatches(structured_gemm(a, w, 1).to(torch.bfloat16), ref) == 0
    seen = {}
    for mutant in ("skip_k", "double_k", "swap_w_in_chunk", "drop_last_chunk"):
        bad = structured_gemm(a, w, 1, mutant, at).to(torch.bfloat16)
        moved = int((bad.float() != structured_gemm(a, w, 1).to(torch.bfloat16).float()).sum())
        seen[mutant] = (_old_close_mismatches(bad, ref), moved)
    print(f"old criterion at {(M, N, Kd)}: (flagged, moved) = {seen}")
    for mutant, (flagged, moved) in seen.items():
        assert moved > 0 and flagged < moved, (mutant, flagged, moved)  # never every moved output
    passes = {m for m, (flagged, _) in seen.items() if flagged == 0}
    assert passes == ({"skip_k", "double_k"} if Kd == 3072 else set())
