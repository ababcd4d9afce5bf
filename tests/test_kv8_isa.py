"""ISA lint of the fp8-KV decode attention (CPU: hipcc cross-compiles to assembly with the production
flags): the instance the batch-128 Phi-3 step runs (D = 96, G = 1) keeps everything in registers."""
from test_isa_lint import _asm, _kernels

HOT = "_Z22decode_attn_kv8_kernelILi96ELi1EE"


def test_kv8_decode_attention_has_no_scratch(tmp_path):
    ks = _kernels(_asm("decode_kv8.hip", tmp_path))
    hits = {n: sc for n, (_, sc) in ks.items() if n.startswith(HOT)}
    assert hits, f"no kernel {HOT}* in decode_kv8.hip (renamed? update the lint): {sorted(ks)[:8]}"
    assert all(sc == 0 for sc in hits.values()), f"scratch in the hot fp8-KV decode kernel: {hits}"
    # the other MHA head dims stay in registers too (GQA groups are correctness-only forms)
    mha = {n: sc for n, (_, sc) in ks.items() if n.startswith("_Z22decode_attn_kv8_kernelILi") and "ELi1EE" in n}
    assert len(mha) == 3 and all(sc == 0 for sc in mha.values()), mha
