"""In-HBM vector indexes (flat brute force, IVFFlat) — the pgvector replacement."""
from __future__ import annotations


def make_index(kind: str, dim: int, device, lists: int = 100, probes: int = 1, capacity: int = 1024,
               dtype: str = "bf16"):
    if dtype not in ("bf16", "fp8"):
        raise ValueError(f"unknown INDEX_DTYPE {dtype!r} (bf16 | fp8)")
    if kind == "flat":
        from .flat import FlatIndex
        return FlatIndex(dim, device, capacity=capacity, dtype=dtype)
    if kind == "ivfflat":
        if dtype != "bf16":
            # IVFFlat permutes and trains on the bf16 rows; an fp8 list store does not exist
            raise ValueError("INDEX_DTYPE=fp8 needs INDEX_KIND=flat")
        from .ivf import IVFFlatIndex
        return IVFFlatIndex(dim, device, lists=lists, probes=probes, capacity=capacity)
    raise ValueError(f"unknown INDEX_KIND {kind!r} (flat | ivfflat)")
