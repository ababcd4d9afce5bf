"""The attention kernels against ops/reference.py on the probe-key inputs of tests/attn_probes.py:
every key of every row is probed in some launch, an included probe reads >= 1.0 and an excluded one
0 (asserted on the reference), so one wrong key is ~50 times the suite's atol = rtol = 0.02.

Each test id names the kernel route its launch takes; _decode_route / _flash_route below restate
the dispatch rules (dec_route in decode_attn.hip, _decode_buffers in ops/kernels.py,
da_flash_attn_v2 in attention.hip) and every test asserts that its shape takes the route it names."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from docagents_amd.ops import kernels as K  # noqa: E402
from docagents_amd.ops import reference as R  # noqa: E402

from attn_probes import DECODE_LENS16, FLASH_LENS, DecodeCase, FlashCase, close, dec_chunk  # noqa: E402

DEV = "cuda"
MAX_SEQ = 4096
MODES = {"uniform": None, "spike4-first": (4.0, ("first",)), "spike10-middle": (10.0, ("middle",)),
         "spike10-last": (10.0, ("last",))}
_REFS: dict = {}


def _decode_route(H, Hkv, D, B, chunk, nsplit, rope, xc_on, fused):
    """(route, xc) of a K.decode_attn launch."""
    pairs, G = B * Hkv, H // Hkv
    xc = bool(fused and nsplit > 1 and H == Hkv and pairs <= 32 and pairs % 8 == 0 and xc_on)
    if G == 1:
        if pairs <= 32 and chunk <= 512:
            return "mfma1", xc
        return ("prefetch" if pairs <= 32 else "stream"), xc
    assert not rope
    return ("gqa-valu" if D == 96 else "gqa-mfma"), False


# id -> (H, Hkv, D, same-XCD exchange, in-kernel merge, chunk arguments, expected route)
DECODE_ROUTES = {
    "mfma1-xc": (2, 2, 96, True, True, [0, 64, 256, 512], "mfma1"),
    "mfma1": (2, 2, 96, False, True, [0, 64, 256, 512], "mfma1"),
    "mfma1-combine": (2, 2, 96, False, False, [0, 64, 256, 512], "mfma1"),
    "mfma1-xc-d64": (2, 2, 64, True, True, [0], "mfma1"),
    "mfma1-xc-d128": (2, 2, 128, True, True, [0], "mfma1"),
    "prefetch-xc": (2, 2, 96, True, True, [1024], "prefetch"),
    "prefetch": (2, 2, 96, False, True, [1024], "prefetch"),
    "prefetch-combine": (2, 2, 96, False, False, [1024], "prefetch"),
    "stream": (4, 4, 96, False, True, [0, 64, 1024], "stream"),
    "stream-combine": (4, 4, 96, False, False, [0, 256], "stream"),
    "gqa-mfma-32-8-128": (32, 8, 128, False, True, [0, 64], "gqa-mfma"),
    "gqa-mfma-32-8-128-combine": (32, 8, 128, False, False, [512], "gqa-mfma"),
    "gqa-valu-8-2-96": (8, 2, 96, False, True, [0, 64], "gqa-valu"),
    "gqa-valu-8-2-96-combine": (8, 2, 96, False, False, [256], "gqa-valu"),
}


def _route_chunks(names):
    return [pytest.param(n, ch, id=f"{n}-chunk{ch}") for n in names for ch in DECODE_ROUTES[n][5]]


def _setup_decode(route, chunk, rope, monkeypatch):
    H, Hkv, D, xc, fused, _, want = DECODE_ROUTES[route]
    monkeypatch.setattr(K, "DECODE_XC", xc)
    monkeypatch.setattr(K, "_FUSED_COMBINE", fused)
    B = len(DECODE_LENS16)
    ch, nsplit = K._decode_split(B, Hkv, MAX_SEQ, chunk)
    assert os.environ.get("DA_DECODE_MFMA1", "1")[:1] != "0", "DA_DECODE_MFMA1=0 reroutes the few-pairs launches"
    xc_ok = xc and K.decode_xc_ok(torch.device(DEV))
    assert xc_ok == xc, "the placement probe refused the same-XCD exchange"
    assert _decode_route(H, Hkv, D, B, ch, nsplit, rope, xc_ok, fused) == (want, xc), "the shape leaves its route"
    # one row of the launch ends on a split boundary: its last split is empty
    assert any(L % dec_chunk(L, nsplit, ch) == 0 and L // dec_chunk(L, nsplit, ch) < nsplit for L in DECODE_LENS16) \
        or nsplit == 1
    return H, Hkv, D


def _run_decode(key, case, call, ref_call):
    refs = _REFS.setdefault(key, {})
    for l in range(case.n_layouts):
        inc = case.layout(l)
        if l not in refs:
            refs[l] = ref_call(case)
            case.check_reference(refs[l], inc, f"{key} layout {l}")
        close(call(case), refs[l], f"layout {l} of {case.n_layouts}")
    case.assert_covered()


def _ref_decode(c):
    k, v = (c.k_cache.clone(), c.v_cache.clone()) if c.rope is not None else (c.k_cache, c.v_cache)
    return R.decode_attn(c.q.clone(), k, v, c.lens, c.slot, c.H, c.Hkv, c.D, pre=c.pre, rope=c.rope)


def _call_decode(chunk):
    def call(c):
        if c.rope is None:
            return K.decode_attn(c.q, c.k_cache, c.v_cache, c.lens, c.slot, c.H, c.Hkv, c.D, MAX_SEQ, chunk=chunk, pre=c.pre)
        k, v = c.k_cache.clone(), c.v_cache.clone()
        got = K.decode_attn(c.q, k, v, c.lens, c.slot, c.H, c.Hkv, c.D, MAX_SEQ, chunk=chunk, pre=c.pre, rope=c.rope)
        s, p = c.slot.long(), c.rope[1].long()
        v_new = c.q.view(c.B, c.H + 2 * c.Hkv, c.D)[:, c.H + c.Hkv:]
        assert torch.equal(v[s, :, p], v_new) and torch.equal(k[s, :, p], c.k_new), "the new token's cache row"
        return got
    return call


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("route,chunk", _route_chunks(list(DECODE_ROUTES)))
def test_decode_probes(route, chunk, mode, monkeypatch):
    H, Hkv, D = _setup_decode(route, chunk, False, monkeypatch)
    c = DecodeCase(H, Hkv, D, DECODE_LENS16, MAX_SEQ, spike=MODES[mode], device=DEV)
    _run_decode(("decode", H, Hkv, D, mode), c, _call_decode(chunk), _ref_decode)


@pytest.mark.parametrize("mode", ["uniform", "spike10-middle"])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("route,chunk", [("mfma1-xc", 0), ("prefetch", 1024), ("stream", 0), ("gqa-mfma-32-8-128", 0),
                                         ("gqa-valu-8-2-96", 0), ("mfma1-combine", 256)])
def test_decode_probes_shared_prefix(route, chunk, P, mode, monkeypatch):
    """pre = (P, slot): keys [0, P) from the prefix slot, key P - 1 the last of them (the row's own slot
    and the prefix slot hold A on the wrong side of P).
    Only the tile that holds key P mixes the two slots; the kernels select its source per key."""
    H, Hkv, D = _setup_decode(route, chunk, False, monkeypatch)
    c = DecodeCase(H, Hkv, D, DECODE_LENS16, MAX_SEQ, pre_P=P, spike=MODES[mode], device=DEV)
    _run_decode(("decode-pre", H, Hkv, D, P, mode), c, _call_decode(chunk), _ref_decode)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("route,chunk", [("mfma1-xc", 0), ("mfma1", 64), ("mfma1-combine", 512), ("prefetch-xc", 1024),
                                         ("prefetch", 1024), ("prefetch-combine", 1024), ("stream", 0),
                                         ("stream-combine", 256)])
def test_decode_probes_fused_rope(route, chunk, mode, monkeypatch):
    """rope = (cos_sin, pos): the new token's k / v (the probe of key lens - 1, a "last" spike) come from
    the qkv row; the cache holds A at that key until the call has written it."""
    H, Hkv, D = _setup_decode(route, chunk, True, monkeypatch)
    c = DecodeCase(H, Hkv, D, DECODE_LENS16, MAX_SEQ, rope=True, spike=MODES[mode], device=DEV)
    _run_decode(("decode-rope", H, Hkv, D, mode), c, _call_decode(chunk), _ref_decode)


# ------------------------------------------------------------------------------ fp8 KV cache
def _quant_cache(x):
    q, s = R.quant_weight_fp8_pow2(x.reshape(-1, x.shape[-1]))
    q, s = q.view(x.shape).contiguous(), s.view(x.shape[:-1]).contiguous()
    assert torch.equal(R.kv8_dequant_all(q, s), x), "the probe rows are not exact in e4m3"
    return q, s


def _kv8_calls(chunk):
    state = {}

    def operands(c):
        if "k" not in state:
            state["k"] = _quant_cache(c.k_cache)
        return state["k"], _quant_cache(c.v_cache)

    def call(c):
        (kq, ks), (vq, vs) = operands(c)
        return K.decode_attn_kv8(c.q, kq, vq, ks, vs, c.lens, c.slot, c.H, c.Hkv, c.D, MAX_SEQ, chunk=chunk, pre=c.pre)

    def ref(c):
        (kq, ks), (vq, vs) = operands(c)
        return R.decode_attn_kv8(c.q, kq, vq, ks, vs, c.lens, c.slot, c.H, c.Hkv, c.D, pre=c.pre)
    return call, ref


KV8_GEOM = {"kv8-mha-2-2-96": (2, 2, 96), "kv8-gqa-32-8-128": (32, 8, 128), "kv8-gqa-8-2-96": (8, 2, 96)}


def _setup_kv8(fused, monkeypatch):
    monkeypatch.setattr(K, "_FUSED_COMBINE", fused)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("fused", [True, False], ids=["merge-in-kernel", "combine"])
@pytest.mark.parametrize("geom,chunk", [("kv8-mha-2-2-96", 0), ("kv8-mha-2-2-96", 64), ("kv8-mha-2-2-96", 256),
                                        ("kv8-mha-2-2-96", 512), ("kv8-gqa-32-8-128", 0), ("kv8-gqa-32-8-128", 64),
                                        ("kv8-gqa-8-2-96", 0), ("kv8-gqa-8-2-96", 256)])
def test_decode_kv8_probes(geom, chunk, fused, mode, monkeypatch):
    _setup_kv8(fused, monkeypatch)
    H, Hkv, D = KV8_GEOM[geom]
    c = DecodeCase(H, Hkv, D, DECODE_LENS16, MAX_SEQ, spike=MODES[mode], device=DEV)
    call, ref = _kv8_calls(chunk)
    _run_decode(("kv8", H, Hkv, D, mode), c, call, ref)


@pytest.mark.parametrize("mode", ["uniform", "spike10-middle"])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("geom", list(KV8_GEOM))
def test_decode_kv8_probes_shared_prefix(geom, P, mode, monkeypatch):
    """As test_decode_probes_shared_prefix, over the fp8 cache (codes and scales of the mixed tile)."""
    _setup_kv8(True, monkeypatch)
    H, Hkv, D = KV8_GEOM[geom]
    c = DecodeCase(H, Hkv, D, DECODE_LENS16, MAX_SEQ, pre_P=P, spike=MODES[mode], device=DEV)
    call, ref = _kv8_calls(0)
    _run_decode(("kv8-pre", H, Hkv, D, P, mode), c, call, ref)


# ----------------------------------------------------------------------------------------- flash
FLASH_MODES = {"uniform": None, "spike4-last": (4.0, ("last",)), "spike10-last": (10.0, ("last",)),
               "spike10-first": (10.0, ("first",)), "spike4-middle+prefix": (4.0, ("middle", "prefix"))}
HEADS = [pytest.param(8, 2, id="gqa-8-2"), pytest.param(4, 4, id="mha-4-4")]


def _flash_route(D, causal, P, aligned=True):
    if causal and D == 96:
        return "pipe-dma" if (P % 64 == 0 and aligned) else "pipe-reg"
    return "v2-8w" if D == 128 else "v2-4w"


def _misaligned_prefix(c):
    """A contiguous [Hkv, S, D] K / V pair 8 bytes off a 16-byte boundary, passed as a prefix of 0 keys:
    the only operand the wrapper accepts misaligned, and the dispatch's alignment test covers it."""
    out = []
    for _ in range(2):
        buf = torch.zeros(c.Hkv * c.S * c.D + 8, dtype=c.q.dtype, device=DEV)
        out.append(buf[4:4 + c.Hkv * c.S * c.D].view(c.Hkv, c.S, c.D))
        assert out[-1].data_ptr() % 16 == 8 and out[-1].is_contiguous()
    return out[0], out[1], 0


def _run_flash(c, call, ref_call=None):
    for l in range(c.n_layouts):
        inc = c.layout(l)
        ref = (ref_call or _ref_flash)(c)
        c.check_reference(ref, inc)
        got = call(c)
        rows = ~torch.isnan(ref.float()[:, 0])  # tail_only: the defined rows
        assert bool(rows.any())
        close(got[rows], ref[rows], f"layout {l} of {c.n_layouts}")
    c.assert_covered()


def _ref_flash(c, **kw):
    return R.flash_attn_varlen(c.q, c.k, c.v, c.cu, c.max_len, c.H, c.Hkv, c.D, c.causal, prefix=c.prefix,
                               kv_cache=c.kv_cache, **kw)


def _call_flash(c, prefix="case", **kw):
    return K.flash_attn_varlen(c.q, c.k, c.v, c.cu, c.max_len, c.H, c.Hkv, c.D, c.causal,
                               prefix=c.prefix if isinstance(prefix, str) else prefix, kv_cache=c.kv_cache, **kw)


@pytest.mark.parametrize("mode", list(FLASH_MODES))
@pytest.mark.parametrize("H,Hkv", HEADS)
@pytest.mark.parametrize("P,aligned,route", [(0, True, "pipe-dma"), (64, True, "pipe-dma"), (128, True, "pipe-dma"),
                                             (1, True, "pipe-reg"), (100, True, "pipe-reg"), (0, False, "pipe-reg")],
                         ids=lambda x: str(x))
def test_flash_probes_pipelined(P, aligned, route, H, Hkv, mode):
    """D = 96 causal: the LDS-DMA form (whole 64-key prefixes, aligned operands) and the register-staged
    form (other prefixes; P = 0 through a misaligned operand)."""
    assert _flash_route(96, True, P, aligned) == route
    c = FlashCase(H, Hkv, 96, FLASH_LENS, P=P, causal=True, spike=FLASH_MODES[mode], device=DEV)
    if aligned:
        _run_flash(c, _call_flash)
    else:
        with pytest.raises(ValueError):  # q / k / v themselves must be 16-B aligned
            K.flash_attn_varlen(c.q, c.qkv[:, H * 96 + 4:(H + Hkv) * 96 + 4], c.v, c.cu, c.max_len, H, Hkv, 96, True)
        mis = _misaligned_prefix(c)
        _run_flash(c, lambda c: _call_flash(c, prefix=mis))


@pytest.mark.parametrize("mode", ["uniform", "spike10-last", "spike4-middle+prefix"])
@pytest.mark.parametrize("H,Hkv", HEADS)
@pytest.mark.parametrize("P", [0, 100])
@pytest.mark.parametrize("D,causal,route", [(96, False, "v2-4w"), (32, True, "v2-4w"), (32, False, "v2-4w"),
                                            (64, True, "v2-4w"), (64, False, "v2-4w"), (128, True, "v2-8w"),
                                            (128, False, "v2-8w")], ids=lambda x: str(x))
def test_flash_probes_v2(D, causal, route, P, H, Hkv, mode):
    assert _flash_route(D, causal, P) == route
    c = FlashCase(H, Hkv, D, FLASH_LENS, P=P, causal=causal, spike=FLASH_MODES[mode], device=DEV)
    _run_flash(c, _call_flash)


@pytest.mark.parametrize("mode", ["uniform", "spike10-last"])
@pytest.mark.parametrize("H,Hkv", HEADS)
@pytest.mark.parametrize("P,route", [(0, "pipe-dma"), (64, "pipe-dma"), (100, "pipe-reg")])
def test_flash_probes_own_keys_from_cache(P, route, H, Hkv, mode):
    """kv_cache=: the sequences' own keys (and their probes) live in their cache slots at pos = P."""
    assert K.flash_kv_cache_ok(96, True) and _flash_route(96, True, P) == route
    c = FlashCase(H, Hkv, 96, FLASH_LENS, P=P, causal=True, spike=FLASH_MODES[mode], from_cache=True, device=DEV)
    _run_flash(c, lambda c: K.flash_attn_varlen(c.q, None, None, c.cu, c.max_len, H, Hkv, 96, True, prefix=c.prefix,
                                                kv_cache=c.kv_cache))


@pytest.mark.parametrize("mode", ["uniform", "spike10-last"])
@pytest.mark.parametrize("D,causal,P,route", [(96, True, 0, "pipe-dma"), (96, True, 100, "pipe-reg"),
                                              (64, True, 0, "v2-4w"), (64, True, 100, "v2-4w"),
                                              (128, False, 0, "v2-8w"), (128, True, 100, "v2-8w")], ids=lambda x: str(x))
def test_flash_probes_tail_only(D, causal, P, route, mode):
    """tail_only=True: the query block holding each sequence's last token, the defined rows only."""
    assert _flash_route(D, causal, P) == route
    c = FlashCase(8, 2, D, FLASH_LENS, P=P, causal=causal, spike=FLASH_MODES[mode], device=DEV)
    out = torch.zeros(c.T, c.H * D, dtype=torch.bfloat16, device=DEV)
    _run_flash(c, lambda c: _call_flash(c, out=out, tail_only=True), lambda c: _ref_flash(c, tail_only=True))


@pytest.mark.parametrize("mode", ["uniform", "spike10-last", "spike4-last"])
@pytest.mark.parametrize("H,Hkv", HEADS)
@pytest.mark.parametrize("causal", [False, True], ids=["bidirectional", "causal"])
@pytest.mark.parametrize("D", [64, 96])
def test_flash_probes_f16(D, causal, H, Hkv, mode):
    """K.flash_attn_f16: the 4-wave flash_attn_v2 kernel in fp16 (A and 0 are exact there too)."""
    c = FlashCase(H, Hkv, D, FLASH_LENS, causal=causal, spike=FLASH_MODES[mode], dtype=torch.float16, device=DEV)
    _run_flash(c, lambda c: K.flash_attn_f16(c.q, c.k, c.v, c.cu, c.max_len, H, Hkv, D, causal),
               lambda c: R.flash_attn_f16(c.q, c.k, c.v, c.cu, c.max_len, H, Hkv, D, causal))
