"""Prefill tail cut on the CPU reference ops: with DA_PREFILL_TAIL on, the last layer's attention, O
projection and MLP run on the rows whose logits are read only. Logits and the whole KV cache must
equal the all-rows path (models/llama.py ``_PREFILL_TAIL``)."""
import numpy as np
import pytest
import torch

from docagents_amd.models import llama
from docagents_amd.models.configs import decoder_config
from docagents_amd.models.llama import LlamaDecoder, pack_prompts

LENS = (1, 2, 127, 128, 129, 300)


@pytest.fixture(scope="module")
def model():
    return LlamaDecoder(decoder_config("tiny-dec"), "cpu", seed=0)


def _prefill(m, tail: bool, P: int):
    """Prefill one pack of LENS-long prompts (after a shared head of P tokens in slot 0 when P > 0);
    returns (logits, a copy of the whole cache, whether the last layer ran cut)."""
    rng = np.random.default_rng(11)
    m.alloc_cache(len(LENS) + 1, 512)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    cuts = []
    routes = m._tail_routes
    m._tail_routes = lambda M: cuts.append(routes(M)) or cuts[-1]
    old = llama._PREFILL_TAIL
    llama._PREFILL_TAIL = tail
    try:
        prefix = None
        if P:
            head = rng.integers(5, 3000, size=P).astype(np.int32)
            m.prefill(t(head), t(np.arange(P, dtype=np.int32)), t(np.zeros(P, dtype=np.int32)),
                      t(np.array([0, P], dtype=np.int32)), P, t(np.array([P - 1], dtype=np.int64)))
            prefix = (0, P)
        prompts = [[int(x) for x in rng.integers(5, 3000, size=n)] for n in LENS]
        flat, pos, cu, lens = pack_prompts(prompts)
        slot_tok = np.repeat(np.arange(1, len(LENS) + 1, dtype=np.int32), lens)
        logits = m.prefill(t(flat), t(pos + P), t(slot_tok), t(cu), int(lens.max()), t((cu[1:] - 1).astype(np.int64)),
                           prefix=prefix)
    finally:
        llama._PREFILL_TAIL = old
        del m._tail_routes
    return logits, m.cache.buf.clone(), cuts[-1] is not None


@pytest.mark.parametrize("P", [0, 64])
def test_tail_cut_equals_all_rows(model, P):
    lg_on, kv_on, cut_on = _prefill(model, True, P)
    lg_off, kv_off, cut_off = _prefill(model, False, P)
    assert cut_on and not cut_off  # the two runs took the two paths
    assert lg_on.shape == (len(LENS), model.cfg.vocab) and torch.isfinite(lg_on.float()).all()
    assert torch.equal(lg_on, lg_off)
    assert torch.equal(kv_on, kv_off)


def test_reference_flash_tail_rows():
    """ops.reference.flash_attn_varlen(tail_only=True): the rows of each sequence's last 128-row
    query block equal the full call's; the rest are undefined (NaN in the oracle)."""
    from docagents_amd.ops import reference as R
    g = torch.Generator().manual_seed(0)
    H, Hkv, D = 4, 2, 32
    cu = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int32)
    T = int(cu[-1])
    q, k, v = (torch.randn((T, n * D), generator=g).to(torch.bfloat16) for n in (H, Hkv, Hkv))
    full = R.flash_attn_varlen(q, k, v, torch.from_numpy(cu), max(LENS), H, Hkv, D, causal=True)
    tail = R.flash_attn_varlen(q, k, v, torch.from_numpy(cu), max(LENS), H, Hkv, D, causal=True, tail_only=True)
    for b, L in enumerate(LENS):
        s0, q0 = int(cu[b]), (L - 1) // 128 * 128
        assert torch.equal(tail[s0 + q0:s0 + L], full[s0 + q0:s0 + L])
        assert torch.isnan(tail[s0:s0 + q0].float()).all()
