"""Framed output buffers for kernel tests: a view for the kernel to write surrounded by rows, pad
columns or guard elements that hold a fixed bit pattern, and bit-exact checks that a launch left
everything outside the view alone.

Every byte of a frame is 0x5A: finite and non-zero in bf16 / fp16 (0x5A5A), fp32 (0x5A5A5A5A) and
e4m3 (0x5A), so a stray store of a plausible result (or of zeros) changes it, and the comparison is
on integers, never on floats. Plain module (no fixtures): works on CPU and GPU tensors alike.
"""
from __future__ import annotations

import torch

PATTERN_BYTE = 0x5A
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _bits(t: torch.Tensor) -> torch.Tensor:
    """``t`` reinterpreted as integers of its element size (same shape and strides)."""
    return t.view(_INT_VIEW[t.element_size()])


def pattern_value(t: torch.Tensor) -> int:
    """The integer one element of a pattern-filled tensor of ``t``'s element size holds."""
    return int.from_bytes(bytes([PATTERN_BYTE]) * t.element_size(), "little")


def fill_pattern(t: torch.Tensor) -> torch.Tensor:
    _bits(t).fill_(pattern_value(t))
    return t


def holds_pattern(t: torch.Tensor) -> bool:
    """True when every element of ``t`` (any view) still has the pattern's bits."""
    return bool((_bits(t) == pattern_value(t)).all())


def framed(M: int, N: int, dtype, col_pad: int, rows_before: int = 8, rows_after: int = 256, device="cpu"):
    """A pattern-filled [rows_before + M + rows_after, N + col_pad] buffer and its view
    [rows_before : rows_before + M, :N] (row stride N + col_pad). col_pad must keep the row stride the
    kernels' wrappers accept: a multiple of 8 elements (16 for one-byte types). rows_after defaults to
    256, the tallest M-tile of the GEMMs: a store to a row past M inside the last tile lands in the
    frame, not beyond the allocation."""
    unit = 16 if torch.empty(0, dtype=dtype).element_size() == 1 else 8
    if col_pad % unit:
        raise ValueError(f"col_pad={col_pad} must be a multiple of {unit} elements for {dtype}")
    buf = fill_pattern(torch.empty((rows_before + M + rows_after, N + col_pad), dtype=dtype, device=device))
    return buf, buf[rows_before:rows_before + M, :N]


def guarded(n: int, dtype, guard: int = 64, device="cpu"):
    """1-D variant for flat outputs: a pattern-filled buffer of guard + n + guard elements and its
    view [guard : guard + n] (contiguous: ``.view(B, k)`` of it is a valid contiguous [B, k] output)."""
    buf = fill_pattern(torch.empty(guard + n + guard, dtype=dtype, device=device))
    return buf, buf[guard:guard + n]


def _view_slices(buffer: torch.Tensor, view) -> tuple:
    if isinstance(view, slice):
        return (view,)
    if isinstance(view, tuple):
        return view
    # a basic-sliced view of ``buffer`` (unit steps): recover its origin from the storage offset
    if view.dim() != buffer.dim() or view.stride() != buffer.stride():
        raise ValueError("view must be a unit-step slice of buffer with the same number of dimensions")
    off = view.storage_offset() - buffer.storage_offset()
    out = []
    for d in range(buffer.dim()):
        st = buffer.stride(d)
        i0, off = (off // st, off % st) if st else (0, off)
        out.append(slice(i0, i0 + view.shape[d]))
    if off:
        raise ValueError("view does not start on an element of buffer")
    return tuple(out)


def assert_frame_intact(buffer: torch.Tensor, view, what: str = "frame") -> None:
    """Every element of ``buffer`` outside ``view`` (a tuple of slices, or the view tensor ``framed`` /
    ``guarded`` returned) still holds the pattern, compared as integers. Reports the number of
    overwritten elements and the first one's index ((row, col) for a 2-D frame)."""
    sl = _view_slices(buffer, view)
    bad = _bits(buffer) != pattern_value(buffer)
    bad[sl] = False
    n = int(bad.sum())
    if n:
        first = tuple(int(i) for i in bad.nonzero()[0])
        inside = tuple((s.start, s.stop) for s in sl)
        raise AssertionError(f"{what}: {n} element(s) outside the view {inside} of a {tuple(buffer.shape)} buffer "
                             f"were overwritten, first at {first}")
