"""Prefill tail cut on the gfx950 kernels: the flash kernels' tail mode, row-subset GEMMs / norms with
the full launch's routing, and the decoder with DA_PREFILL_TAIL on and off. Everything is compared
bit for bit: the cut removes work, it does not change a single stored value that is read."""
import numpy as np

import pytest
import torch

pytestmark = pytest.mark.gpu

from docagents_amd.models import llama  # noqa: E402
from docagents_amd.models.configs import DecoderConfig, decoder_config  # noqa: E402
from docagents_amd.models.llama import LlamaDecoder, pack_prompts  # noqa: E402
from docagents_amd.ops import kernels as K  # noqa: E402

DEV = "cuda"
SENTINEL = 777.0


def _rand(*shape, scale=1.0):
    return (torch.randn(*shape, device=DEV) * scale).to(torch.bfloat16)


# ------------------------------------------------------------------------------ flash tail mode
FLASH_LENS = (1, 127, 128, 129, 257, 300)


def _flash_case(H, Hkv, D, P, from_cache, lens=FLASH_LENS):
    """(full output, tail-mode output over a sentinel-filled buffer, cu) of one pack: sequence b's own
    keys at cache[b, :, P + j], the shared prefix in the last slot."""
    torch.manual_seed(1000 * D + 10 * P + from_cache)
    S, Lmax, T = len(lens) + 1, 512, sum(lens)
    kc, vc = _rand(S, Hkv, Lmax, D), _rand(S, Hkv, Lmax, D)
    q = _rand(T, H * D)
    cu = torch.tensor([0] + list(np.cumsum(lens)), device=DEV, dtype=torch.int32)
    slot = torch.cat([torch.full((n,), b, dtype=torch.int32) for b, n in enumerate(lens)]).to(DEV)
    pos = torch.cat([torch.arange(P, P + n, dtype=torch.int32) for n in lens]).to(DEV)
    pre = (kc[S - 1], vc[S - 1], P) if P else None
    if from_cache:
        kw = dict(kv_cache=(kc, vc, slot, pos))
        k = v = None
    else:
        kw = {}
        k = torch.cat([kc[b, :, P:P + n].transpose(0, 1).reshape(n, Hkv * D) for b, n in enumerate(lens)])
        v = torch.cat([vc[b, :, P:P + n].transpose(0, 1).reshape(n, Hkv * D) for b, n in enumerate(lens)])
    full = K.flash_attn_varlen(q, k, v, cu, max(lens), H, Hkv, D, True, prefix=pre, **kw)
    out = torch.full((T, H * D), SENTINEL, dtype=torch.bfloat16, device=DEV)
    tail = K.flash_attn_varlen(q, k, v, cu, max(lens), H, Hkv, D, True, prefix=pre, out=out, tail_only=True, **kw)
    assert tail.data_ptr() == out.data_ptr()
    return full, tail, cu.tolist()


def _check_tail(full, tail, cu, lens, block):
    assert torch.isfinite(full.float()).all()
    for b, L in enumerate(lens):
        s0, q0 = cu[b], (L - 1) // block * block
        assert torch.equal(tail[s0 + q0:s0 + L], full[s0 + q0:s0 + L]), f"sequence {b}: last block differs"
        assert bool((tail[s0:s0 + q0] == SENTINEL).all()), f"sequence {b}: a row outside the last block was written"


# P = 40: the prefix is no whole 64-key tile, so the launcher takes the non-DMA pipe instantiation
@pytest.mark.parametrize("P", [0, 64, 40])
@pytest.mark.parametrize("from_cache", [False, True])
def test_flash_tail_mode_pipe(P, from_cache):
    """D = 96 causal (flash_attn_pipe_kernel, DMA and non-DMA): only each sequence's last 128-row
    query block is stored, with the full launch's bits; every other row keeps the sentinel."""
    full, tail, cu = _flash_case(4, 4, 96, P, from_cache)
    _check_tail(full, tail, cu, FLASH_LENS, 128)


@pytest.mark.parametrize("H,Hkv,D,block", [(4, 2, 64, 128), (4, 2, 128, 256), (8, 8, 64, 128)])
@pytest.mark.parametrize("P", [0, 64])
def test_flash_tail_mode_v2(H, Hkv, D, block, P):
    """flash_attn_v2_kernel (D = 64: 4 waves, 128-row blocks; D = 128: 8 waves, 256-row blocks), with
    and without fa_block's XCD grouping ((Hkv * B) % 8 == 0 at 8 kv heads x 6 sequences)."""
    full, tail, cu = _flash_case(H, Hkv, D, P, False)
    _check_tail(full, tail, cu, FLASH_LENS, block)


def test_flash_tail_mode_xcd_grouped_pipe():
    """8 sequences x 4 kv heads: fa_block's XCD-grouped order on the one-block-wide tail grid."""
    lens = (300, 1, 129, 257, 128, 64, 200, 31)
    full, tail, cu = _flash_case(4, 4, 96, 64, True, lens=lens)
    _check_tail(full, tail, cu, lens, 128)


# --------------------------------------------------------------------------- row-subset GEMMs
def _idx_sets(M):
    """Row subsets of 1, 3 and 37 rows; the larger ones hold rows of the first and the last row tile
    (row 0 and row M - 1), the single rows are one of each."""
    g = torch.Generator().manual_seed(M)
    sets = [torch.tensor([0]), torch.tensor([M - 1])]
    for n in (3, 37):
        mid = torch.randperm(M - 2, generator=g)[:n - 2] + 1
        sets.append(torch.cat([torch.tensor([0, M - 1]), mid]).sort().values)
    return [s.to(DEV) for s in sets]


def _subset_equals_full(a, w, epi, idx, route, resid=None):
    full = K.gemm(a, w, epi=epi, resid=resid)
    forced = K.gemm(a, w, epi=epi, resid=resid, **route)
    assert torch.equal(full, forced)  # the route IS what the full launch runs
    for ix in idx:
        sub = K.gemm(a.index_select(0, ix), w, epi=epi, resid=None if resid is None else resid.index_select(0, ix),
                     **route)
        assert sub.shape[0] == ix.numel()
        assert torch.equal(sub, full.index_select(0, ix)), f"{ix.numel()} rows, route {route}"


@pytest.mark.parametrize("M", [300, 700])
@pytest.mark.parametrize("N,Kd", [(512, 3072), (256, 8192)])
@pytest.mark.parametrize("epi", [K.EPI_NONE, K.EPI_RESID, K.EPI_SWIGLU])
def test_row_subset_gemm_has_full_launch_bits(M, N, Kd, epi):
    torch.manual_seed(M + N + epi)
    a, w = _rand(M, Kd), _rand(N, Kd, scale=Kd ** -0.5)
    resid = _rand(M, N) if epi == K.EPI_RESID else None
    route = K.gemm_route(M, N, Kd, epi)
    assert route is not None and route["tile"] in (1, 2, 7, 10)
    _subset_equals_full(a, w, epi, _idx_sets(M), route, resid)


@pytest.mark.parametrize("tile", [1, 7, 10])
@pytest.mark.parametrize("epi", [K.EPI_NONE, K.EPI_RESID, K.EPI_SWIGLU])
def test_row_subset_gemm_every_prefill_tile(tile, epi):
    """The tiles gemm_route returns only at other shapes (256-row gemm8p from ~half a chip of tiles,
    128x128 for K < 128) and the 128-row gemm8p, forced: M smaller than the tile's row height."""
    torch.manual_seed(tile)
    M, N, Kd = 700, 512, 3072
    a, w = _rand(M, Kd), _rand(N, Kd, scale=Kd ** -0.5)
    resid = _rand(M, N) if epi == K.EPI_RESID else None
    route = {"tile": tile, "splits": 1}
    full = K.gemm(a, w, epi=epi, resid=resid, **route)
    for ix in _idx_sets(M):
        sub = K.gemm(a.index_select(0, ix), w, epi=epi, resid=None if resid is None else resid.index_select(0, ix),
                     **route)
        assert torch.equal(sub, full.index_select(0, ix))


def test_gemm_route_small_m_is_none():
    assert K.gemm_route(128, 512, 3072) is None and K.gemm_route(1, 512, 3072) is None
    assert K.gemm_route(129, 512, 3072)["tile"] == 2


@pytest.mark.parametrize("M", [300, 1500])
def test_row_subset_rmsnorm_has_full_launch_bits(M):
    """rmsnorm picks its kernel by row count (one wave per row from 1024 rows): route_m gives a
    subset the same kernel, hence the same sum order."""
    torch.manual_seed(M)
    x, g = _rand(M, 3072), _rand(3072)
    full = K.rmsnorm(x, g, 1e-5)
    for ix in _idx_sets(M):
        assert torch.equal(K.rmsnorm(x.index_select(0, ix), g, 1e-5, route_m=M), full.index_select(0, ix))


# ------------------------------------------------------------------------------------ decoder
MHA96 = DecoderConfig("tiny-mha96", vocab=32064, hidden=768, layers=2, heads=8, kv_heads=8, ffn=1024,
                      max_pos=4096, rope_theta=10000.0)  # Phi-3's head shape (D = 96, MHA)
DEC_LENS = (100, 127, 128, 129, 255, 256, 257, 300)


@pytest.fixture(scope="module", params=["mha96", "gqa64"])
def model(request):
    cfg = MHA96 if request.param == "mha96" else decoder_config("tiny-dec")
    return LlamaDecoder(cfg, DEV, seed=0)


def _prompts(shared: int):
    rng = np.random.default_rng(5)
    head = [int(t) for t in rng.integers(5, 3000, size=shared)]
    return [head + [int(t) for t in rng.integers(5, 3000, size=n)] for n in DEC_LENS]


def _prefill(m, tail, P):
    """One packed prefill (after the shared head of P tokens into slot 0); logits + the cache."""
    old, llama._PREFILL_TAIL = llama._PREFILL_TAIL, tail
    try:
        m.alloc_cache(len(DEC_LENS) + 1, 1024)
        prompts = _prompts(P)
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
        prefix = None
        if P:
            m.prefill(to(np.asarray(prompts[0][:P], dtype=np.int32)), to(np.arange(P, dtype=np.int32)),
                      to(np.zeros(P, dtype=np.int32)), to(np.array([0, P], dtype=np.int32)), P,
                      to(np.array([P - 1], dtype=np.int64)))
            prefix = (0, P)
        flat, pos, cu, lens = pack_prompts([p[P:] for p in prompts])
        slot_tok = np.repeat(np.arange(1, len(DEC_LENS) + 1, dtype=np.int32), lens)
        assert (m._tail_routes(len(flat)) is not None) == tail
        logits = m.prefill(to(flat), to(pos + P), to(slot_tok), to(cu), int(lens.max()),
                           to((cu[1:] - 1).astype(np.int64)), prefix=prefix)
        torch.cuda.synchronize()
        return logits.clone(), m.cache.buf.clone()
    finally:
        llama._PREFILL_TAIL = old


@pytest.mark.parametrize("P", [0, 64])
def test_decoder_prefill_tail_bit_identical(model, P):
    lg_on, kv_on = _prefill(model, True, P)
    lg_off, kv_off = _prefill(model, False, P)
    assert torch.isfinite(lg_on.float()).all()
    assert torch.equal(lg_on, lg_off)
    assert torch.equal(kv_on, kv_off)


@pytest.mark.parametrize("share", [False, True])
def test_decoder_greedy_decode_after_tail_prefill(model, share):
    """Twenty greedy tokens per prompt through the generator (prefill + decode), flag on and off."""
    from docagents_amd.engine.generator import Generator
    toks = {}
    for tail in (True, False):
        old, llama._PREFILL_TAIL = llama._PREFILL_TAIL, tail
        try:
            model.cache = None  # a fresh cache per run: the rows' slots, the dummy slot and the head's
            g = Generator(model, max_batch=len(DEC_LENS) + 1, max_seq=1024, temperature=0.0, use_graphs=False,
                          share_prefix=share)
            toks[tail] = [r.tokens for r in g.generate(_prompts(64), 20)]
        finally:
            llama._PREFILL_TAIL = old
    assert all(len(t) == 20 for t in toks[True])
    assert toks[True] == toks[False]
