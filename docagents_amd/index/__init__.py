"""In-HBM vector indexes (flat brute force, IVFFlat) — the pgvector replacement."""
from __future__ import annotations

INDEX_KINDS = ("flat", "ivfflat", "ivfflat_fp8")


def index_row_dtype(kind: str, dtype: str = "bf16") -> str:
    """The row storage of an index of ``kind`` under INDEX_DTYPE=``dtype``: ivfflat_fp8 names its own
    (fp8, whatever INDEX_DTYPE says); the other kinds store what INDEX_DTYPE says."""
    return "fp8" if kind == "ivfflat_fp8" else dtype


def make_index(kind: str, dim: int, device, lists: int = 100, probes: int = 1, capacity: int = 1024,
               dtype: str = "bf16"):
    if dtype not in ("bf16", "fp8"):
        raise ValueError(f"unknown INDEX_DTYPE {dtype!r} (bf16 | fp8)")
    if kind == "flat":
        from .flat import FlatIndex
        return FlatIndex(dim, device, capacity=capacity, dtype=dtype)
    if kind == "ivfflat":
        if dtype != "bf16":
            # INDEX_DTYPE is the flat index's storage; the fp8 IVFFlat index is a kind of its own
            raise ValueError("INDEX_DTYPE=fp8 needs INDEX_KIND=flat")
        from .ivf import IVFFlatIndex
        return IVFFlatIndex(dim, device, lists=lists, probes=probes, capacity=capacity)
    if kind == "ivfflat_fp8":
        from .ivf import IVFFlatIndex
        return IVFFlatIndex(dim, device, lists=lists, probes=probes, capacity=capacity, dtype="fp8")
    raise ValueError(f"unknown INDEX_KIND {kind!r} ({' | '.join(INDEX_KINDS)})")
