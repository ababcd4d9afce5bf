"""tests/kernel_frames.py is not vacuous: a correct write passes, a one-element stray write anywhere
in the frame fails and is located (CPU tensors; the GPU suite uses the same code on device tensors)."""
import pytest
import torch

from kernel_frames import (PATTERN_BYTE, assert_frame_intact, fill_pattern, framed, guarded, holds_pattern,
                           pattern_value)

DTYPES = [torch.bfloat16, torch.float16, torch.float32, torch.float8_e4m3fn, torch.int32]


def _pad(dtype):
    return 16 if dtype == torch.float8_e4m3fn else 8


def _one(dtype, v=1.0):
    return torch.tensor(v).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pattern_is_finite_nonzero_and_every_byte(dtype):
    buf, view = framed(5, 24, dtype, _pad(dtype), rows_before=2, rows_after=3)
    assert buf.shape == (10, 24 + _pad(dtype)) and view.shape == (5, 24) and view.stride(0) == 24 + _pad(dtype)
    assert bool((buf.view(torch.uint8) == PATTERN_BYTE).all())
    f = buf.float()
    assert bool(torch.isfinite(f).all()) and bool((f != 0).all())
    assert holds_pattern(buf) and holds_pattern(view)
    assert pattern_value(buf) == int.from_bytes(bytes([PATTERN_BYTE]) * buf.element_size(), "little")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("extra", [0, 16])
def test_correct_write_passes(dtype, extra):
    pad = _pad(dtype) + extra
    buf, view = framed(7, 40, dtype, pad)
    assert buf.shape == (8 + 7 + 256, 40 + pad)
    view.copy_(torch.arange(7 * 40).reshape(7, 40).remainder(97).to(dtype))
    assert_frame_intact(buf, view)
    assert_frame_intact(buf, (slice(8, 15), slice(0, 40)))
    assert not holds_pattern(view)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("where", ["row_before", "row_after", "pad_column", "last_element"])
def test_one_stray_element_fails_and_is_located(dtype, where):
    M, N, pad = 7, 40, _pad(dtype)
    buf, view = framed(M, N, dtype, pad)
    view.fill_(_one(dtype))
    r, c = {"row_before": (7, 3), "row_after": (8 + M, N - 1), "pad_column": (8 + M - 1, N),
            "last_element": (buf.shape[0] - 1, buf.shape[1] - 1)}[where]
    buf[r, c] = _one(dtype, 0.0)  # zero is a plausible stray store and differs from the pattern
    with pytest.raises(AssertionError, match=rf"1 element\(s\).*first at \({r}, {c}\)"):
        assert_frame_intact(buf, view)
    with pytest.raises(AssertionError):
        assert_frame_intact(buf, (slice(8, 8 + M), slice(0, N)))


def test_count_and_first_offender():
    buf, view = framed(4, 16, torch.bfloat16, 8)
    buf[100, 5] = 1.0
    buf[3, 20] = 1.0
    buf[3, 21] = 1.0
    with pytest.raises(AssertionError, match=r"3 element\(s\).*first at \(3, 20\)"):
        assert_frame_intact(buf, view)


def test_bits_not_values():
    """The comparison is on bits: a value equal to the pattern as a float but not in bits (-0.0 vs 0.0
    cannot arise with this pattern; a NaN written over it must still be seen) is reported."""
    buf, view = framed(2, 8, torch.float32, 8)
    buf[0, 0] = float("nan")
    with pytest.raises(AssertionError, match=r"first at \(0, 0\)"):
        assert_frame_intact(buf, view)
    buf2, view2 = framed(2, 8, torch.bfloat16, 8)
    near = buf2[0, 0].float().item() * (1 + 2.0 ** -7)  # one bf16 ulp away from the pattern's value
    buf2[0, 1] = near
    with pytest.raises(AssertionError, match=r"first at \(0, 1\)"):
        assert_frame_intact(buf2, view2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32, torch.bfloat16])
def test_guarded_flat_outputs(dtype):
    buf, view = guarded(10, dtype, guard=4)
    assert buf.shape == (18,) and view.shape == (10,) and view.is_contiguous()
    view.view(5, 2).copy_(torch.arange(10).reshape(5, 2).to(dtype))  # a [B, 2] output inside the guards
    assert_frame_intact(buf, view)
    assert_frame_intact(buf, slice(4, 14))
    for i in (3, 14, 17, 0):
        b2, v2 = guarded(10, dtype, guard=4)
        b2[i] = 0
        with pytest.raises(AssertionError, match=rf"first at \({i},\)"):
            assert_frame_intact(b2, v2)


def test_col_pad_must_keep_the_wrappers_stride_rule():
    with pytest.raises(ValueError):
        framed(4, 16, torch.bfloat16, 4)
    with pytest.raises(ValueError):
        framed(4, 16, torch.float8_e4m3fn, 8)
    framed(4, 16, torch.float8_e4m3fn, 16)


def test_fill_pattern_on_a_view_marks_rows_unwritten():
    """A framed view pre-filled with the pattern (outputs a kernel writes only in part): rows that
    were written differ, the others still hold it."""
    buf, view = framed(6, 8, torch.bfloat16, 8)
    fill_pattern(view)
    view[4:] = 0.5
    assert holds_pattern(view[:4]) and not holds_pattern(view[4:])
    assert_frame_intact(buf, view)
