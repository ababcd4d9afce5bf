"""The probe-key inputs of tests/attn_probes.py bite: on them the unmodified reference satisfies the
builders' conditions (included probes >= 1.0, everything else 0, no key unprobed), and each
deliberately wrong attention below falls outside the suite's atol = rtol = 0.02 against it.
Runs on the CPU with ops/reference.py alone."""
import math

import pytest
import torch

from docagents_amd.ops import reference as R

from attn_probes import (DECODE_LENS, FLASH_LENS, DecodeCase, FlashCase, close, dec_chunk, mismatches, pow2ceil,
                         rope_table_90, spike_kappa)

H, HKV, D = 2, 2, 64
BIG = DECODE_LENS.index(2935)


def _decode_ref(c, lens=None, k=None, v=None, pre="case", q=None):
    rope = c.rope
    k = c.k_cache if k is None else k
    v = c.v_cache if v is None else v
    if rope is not None:
        k, v = k.clone(), v.clone()
    return R.decode_attn((c.q if q is None else q).clone(), k, v, c.lens if lens is None else lens, c.slot, c.H, c.Hkv,
                         c.D, pre=c.pre if isinstance(pre, str) else pre, rope=rope)


def _rejected(case, mutant, rows=None):
    """True when the mutant's output misses the criterion against the reference in some layout, for
    every row of ``rows`` (default: at least one row); checks the reference's conditions on the way."""
    hit = torch.zeros(case.B, dtype=torch.bool)
    for l in range(case.n_layouts):
        inc = case.layout(l)
        ref = _decode_ref(case)
        case.check_reference(ref, inc)
        got = mutant(case)
        for b in range(case.B):
            hit[b] |= mismatches(got[b], ref[b]) > 0
    case.assert_covered()
    return bool(hit.any()) if rows is None else bool(hit[rows].all())


@pytest.mark.parametrize("mode", ["uniform", "spike4", "spike10", "rope", "rope-spike", "pre65"])
def test_decode_reference_meets_the_conditions(mode):
    kw = {"uniform": {}, "spike4": dict(spike=(4.0, ("first", "last"))), "spike10": dict(spike=(10.0, ("middle",))),
          "rope": dict(rope=True), "rope-spike": dict(rope=True, spike=(10.0, ("first", "last"))),
          "pre65": dict(pre_P=65)}[mode]
    c = DecodeCase(H, HKV, D, DECODE_LENS, **kw)
    assert c.A == pow2ceil(c.A) and c.A >= max(DECODE_LENS)
    for l in range(c.n_layouts):
        inc = c.layout(l)
        ref = _decode_ref(c)
        c.check_reference(ref, inc)
        assert mismatches(ref, ref) == 0
    c.assert_covered()


def test_rope_table_90_is_exact():
    cs = rope_table_90(64, D)
    x = torch.randn(64, 3, D).to(torch.bfloat16)
    y = R._rope_rows(x, cs).to(torch.bfloat16)
    assert torch.equal(y.float().abs().sort(-1).values, x.float().abs().sort(-1).values)
    assert spike_kappa(10.0, 96) == (24.0, 4 * 24.0 / math.sqrt(96)) and spike_kappa(4.0, 96)[0] == 10.0


def test_mutant_decode_lens_plus_one():
    c = DecodeCase(H, HKV, D, DECODE_LENS)
    assert _rejected(c, lambda c: _decode_ref(c, lens=c.lens + 1), rows=slice(None))


def test_mutant_decode_lens_minus_one():
    c = DecodeCase(H, HKV, D, DECODE_LENS)
    rows = [b for b, L in enumerate(DECODE_LENS) if L > 1]
    assert _rejected(c, lambda c: _decode_ref(c, lens=(c.lens - 1).clamp_min(1)), rows=rows)


def test_mutant_decode_v_tile_zeroed():
    c = DecodeCase(H, HKV, D, DECODE_LENS)

    def mutant(c):
        v = c.v_cache.clone()
        v[c.slot_l[BIG], :, 1024:1088] = 0
        return _decode_ref(c, v=v)
    assert _rejected(c, mutant, rows=[BIG])


def test_mutant_decode_tile_from_neighbouring_slot():
    c = DecodeCase(H, HKV, D, DECODE_LENS)

    def mutant(c):
        k, v = c.k_cache.clone(), c.v_cache.clone()
        s = c.slot_l[BIG]
        k[s, :, 1024:1088], v[s, :, 1024:1088] = k[s - 1, :, 1024:1088], v[s - 1, :, 1024:1088]
        return _decode_ref(c, k=k, v=v)
    assert _rejected(c, mutant, rows=[BIG])


@pytest.mark.parametrize("P", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("which", ["last prefix key from the own slot", "first own key from the prefix slot"])
def test_mutant_decode_prefix_boundary(P, which):
    c = DecodeCase(H, HKV, D, DECODE_LENS, pre_P=P)
    rows = [b for b, p in enumerate(c.P_l) if p and (which.startswith("last") or c.lens_l[b] > p)]
    assert rows

    def mutant(c):  # the row's keys gathered into its own slot, one key from the wrong side
        k, v = c.k_cache.clone(), c.v_cache.clone()
        for b in rows:
            s = c.slot_l[b]
            for t, t0 in ((k, c.k_cache), (v, c.v_cache)):
                t[s, :, :P] = t0[c.pslot, :, :P]
                if which.startswith("last"):
                    t[s, :, P - 1] = t0[s, :, P - 1]
                else:
                    t[s, :, P] = t0[c.pslot, :, P]
        return _decode_ref(c, k=k, v=v, pre=None)
    assert _rejected(c, mutant, rows=rows)


@pytest.mark.parametrize("spike", [None, (10.0, ("last",))])
def test_mutant_decode_new_token_dropped(spike):
    c = DecodeCase(H, HKV, D, DECODE_LENS, rope=True, spike=spike)
    rows = [b for b, L in enumerate(DECODE_LENS) if L > 1]

    def mutant(c):  # the cache holds the new token, the softmax leaves its term out
        k, v = c.k_cache.clone(), c.v_cache.clone()
        q = R.rope_cache(c.q.clone(), c.rope[1], c.rope[0], c.H, c.Hkv, c.D, slot=c.slot, k_cache=k, v_cache=v)
        return R.decode_attn(q, k, v, (c.lens - 1).clamp_min(1), c.slot, c.H, c.Hkv, c.D)
    assert _rejected(c, mutant, rows=rows)


def _split_merge(c, nsplit, chunk, weight=None, omit=None, row=BIG):
    """decode attention as the kernels organise it: per split (max, sum, unnormalised O) partials of
    the balanced splits, combined in fp64. weight = (split, factor) / omit = split mutate ``row``."""
    out = torch.zeros(c.B, c.H * c.D, dtype=torch.float64)
    G = c.H // c.Hkv
    scale = 1.0 / math.sqrt(c.D)
    for b in range(c.B):
        L, s = c.lens_l[b], c.slot_l[b]
        q = c.q[b, :c.H * c.D].double().view(c.H, 1, c.D)
        kk = c.k_cache[s, :, :L].double().repeat_interleave(G, 0)
        vv = c.v_cache[s, :, :L].double().repeat_interleave(G, 0)
        sc = (q @ kk.transpose(1, 2)) * scale  # [H, 1, L]
        ch = dec_chunk(L, nsplit, chunk)
        parts = []
        for i in range(nsplit):
            k0, k1 = i * ch, min(L, (i + 1) * ch)
            if k1 <= k0 or (b == row and omit == i):
                continue
            m = sc[..., k0:k1].amax(-1, keepdim=True)
            p = (sc[..., k0:k1] - m).exp()
            f = weight[1] if (weight is not None and b == row and weight[0] == i) else 1.0
            parts.append((m, p.sum(-1, keepdim=True), p @ vv[:, k0:k1], f))
        M = torch.stack([p[0] for p in parts]).amax(0)
        lsum = sum(p[1] * (p[0] - M).exp() * p[3] for p in parts)
        acc = sum(p[2] * (p[0] - M).exp() * p[3] for p in parts)
        out[b] = (acc / lsum).reshape(-1)
    return out.to(torch.bfloat16)


@pytest.mark.parametrize("beta,where", [(4.0, "first"), (10.0, "middle"), (10.0, "last")])
def test_mutant_decode_split_merge(beta, where):
    """Spike mode: the splits' maxima differ, so a wrong merge weight or a lost split shows."""
    nsplit, chunk = 8, 512
    c = DecodeCase(H, HKV, D, DECODE_LENS, spike=(beta, (where,)))
    ch = dec_chunk(2935, nsplit, chunk)
    spike_split = c.spikes[BIG][0] // ch
    other = (spike_split + 3) % 6
    for l in range(c.n_layouts):  # the unmutated merge is the reference
        c.layout(l)
        close(_split_merge(c, nsplit, chunk), _decode_ref(c), "fp64 split merge")
    for mut in (dict(weight=(spike_split, 2.0)), dict(weight=(spike_split, 0.5)), dict(weight=(other, 2.0)),
                dict(weight=(other, 0.5)), dict(omit=spike_split), dict(omit=other)):
        assert _rejected(c, lambda c: _split_merge(c, nsplit, chunk, **mut), rows=[BIG]), mut


# ----------------------------------------------------------------------------------------- flash
FH, FHKV, FD = 4, 2, 32
LONG = FLASH_LENS.index(385)


def _flash_ref(c):
    return R.flash_attn_varlen(c.q, c.k, c.v, c.cu, c.max_len, c.H, c.Hkv, c.D, c.causal, prefix=c.prefix,
                               kv_cache=c.kv_cache)


def _flash_masked(c, edit=None):
    """Causal attention with an explicit visibility mask [L, P + L] per sequence, which ``edit(b, mask)``
    may change (True = visible); fp32 like the reference."""
    G, P = c.H // c.Hkv, c.P
    out = torch.empty(c.T, c.H * c.D, dtype=c.q.dtype)
    for b, L in enumerate(c.lens_l):
        s0 = c.cu_l[b]
        q = c.q[s0:s0 + L].float().view(L, c.H, c.D).transpose(0, 1)
        k = c.k[s0:s0 + L].float().view(L, c.Hkv, c.D).transpose(0, 1)
        v = c.v[s0:s0 + L].float().view(L, c.Hkv, c.D).transpose(0, 1)
        if P:
            k, v = torch.cat([c.prefix[0][:, :P].float(), k], 1), torch.cat([c.prefix[1][:, :P].float(), v], 1)
        k, v = k.repeat_interleave(G, 0), v.repeat_interleave(G, 0)
        vis = torch.ones(L, P + L, dtype=torch.bool).tril(P)
        if edit is not None:
            edit(b, vis)
        s = (q @ k.transpose(1, 2)) / math.sqrt(c.D)
        p = s.masked_fill(~vis, float("-inf")).softmax(-1)
        out[s0:s0 + L] = (p @ v).transpose(0, 1).reshape(L, c.H * c.D).to(out.dtype)
    return out


def _flash_rejected(c, edit, rows):
    hit = torch.zeros(c.T, dtype=torch.bool)
    for l in range(c.n_layouts):
        inc = c.layout(l)
        ref = _flash_ref(c)
        c.check_reference(ref, inc)
        close(_flash_masked(c), ref, "unmutated mask")
        got = _flash_masked(c, edit)
        hit |= (~((got.float() - ref.float()).abs() <= 0.02 + 0.02 * ref.float().abs())).any(-1)
    c.assert_covered()
    other = torch.ones(c.T, dtype=torch.bool)
    other[rows] = False
    return bool(hit[rows].all()) and not bool(hit[other].any())


@pytest.mark.parametrize("kw", [dict(), dict(P=100), dict(causal=False), dict(P=64, spike=(10.0, ("last", "prefix"))),
                                dict(spike=(4.0, ("first", "middle"))), dict(P=64, from_cache=True),
                                dict(dtype=torch.float16, spike=(10.0, ("middle",)))],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()) or "plain")
def test_flash_reference_meets_the_conditions(kw):
    c = FlashCase(FH, FHKV, FD, FLASH_LENS, **kw)
    for l in range(c.n_layouts):
        inc = c.layout(l)
        ref = _flash_ref(c) if c.q.dtype == torch.bfloat16 else R.flash_attn_f16(
            c.q, c.k, c.v, c.cu, c.max_len, c.H, c.Hkv, c.D, c.causal)
        c.check_reference(ref, inc)
    c.assert_covered()


@pytest.mark.parametrize("P", [0, 100])
@pytest.mark.parametrize("shift", [1, -1])
def test_mutant_flash_diagonal_on_long_rows(P, shift):
    """The causal diagonal moved by one key, for rows >= 256 of one sequence only."""
    c = FlashCase(FH, FHKV, FD, FLASH_LENS, P=P)
    L = FLASH_LENS[LONG]

    def edit(b, vis):
        if b == LONG:
            vis[256:] = torch.ones(L, P + L, dtype=torch.bool).tril(P + shift)[256:]
    rows = [c.cu_l[LONG] + i for i in range(256, L - (1 if shift > 0 else 0))]  # the last row has no key P + L
    assert _flash_rejected(c, edit, rows)


@pytest.mark.parametrize("P", [0, 64])
def test_mutant_flash_tile_skipped_for_one_query_block(P):
    c = FlashCase(FH, FHKV, FD, FLASH_LENS, P=P)

    def edit(b, vis):
        if b == LONG:
            vis[128:256, 64:128] = False
    assert _flash_rejected(c, edit, [c.cu_l[LONG] + i for i in range(128, 256)])
