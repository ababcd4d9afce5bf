"""CPU checks of the vector index's host logic and of the reference ops the CPU index runs on."""
import numpy as np
import pytest
import torch

from docagents_amd.index.flat import FlatIndex
from docagents_amd.ops import reference as R

from topk_cases import MERGE_K, MERGE_P, MERGE_Q, assert_merge, merge_case


@pytest.mark.parametrize("K", MERGE_K)
@pytest.mark.parametrize("Q", MERGE_Q)
@pytest.mark.parametrize("P", MERGE_P)
def test_reference_topk_merge_is_lexicographic(P, Q, K):
    """reference.topk_merge orders as the kernel's better(): score descending, id ascending, empties
    last, also where two scores are one fp32 ulp apart under ids 1e8 apart."""
    cs, ci = merge_case(P, Q, K)
    keep_s, keep_i = cs.clone(), ci.clone()
    s, i = R.topk_merge(cs, ci, K)
    assert_merge(s, i, keep_s, keep_i, K)
    assert torch.equal(cs.view(torch.int32), keep_s.view(torch.int32)) and torch.equal(ci, keep_i)


def test_reference_topk_merge_one_ulp_against_a_large_id():
    half = np.float32(0.5)
    up = float(np.nextafter(half, np.float32(1)))
    cs = torch.tensor([[[0.5, 0.25]], [[up, 0.5]]])                       # [P = 2, Q = 1, K = 2]
    ci = torch.tensor([[[3, 1]], [[99_999_937, 70_000_000]]], dtype=torch.int32)
    s, i = R.topk_merge(cs, ci, 2)
    assert i.tolist() == [[99_999_937, 3]] and s.tolist() == [[up, 0.5]]
    s, i = R.topk_merge(cs, ci.clone().fill_(-1), 2)
    assert i.tolist() == [[-1, -1]] and bool(torch.isneginf(s).all())


def _flat(n_docs=4, rows=10, d=32):
    g = torch.Generator().manual_seed(0)
    X = torch.nn.functional.normalize(torch.randn(n_docs * rows, d, generator=g), dim=-1)
    ix = FlatIndex(d, "cpu")
    for i in range(n_docs):
        ix.add(f"d{i}", np.arange(rows * i, rows * (i + 1)), X[rows * i:rows * (i + 1)])
    return ix, X


def test_ranges_for_names_each_document_once():
    """A filter that names a document twice gets its ranges once and counts its rows once (the range
    scan walks the concatenated ranges: a repeated range is a repeated row in the top-k)."""
    ix, _ = _flat()
    ix.add("d0", np.arange(100, 105), torch.nn.functional.normalize(torch.randn(5, 32), dim=-1))  # second range
    assert ix._ranges_for([["d0", "d0"]]) == ix._ranges_for([["d0"]]) == ([(0, 10), (40, 45)], [0, 2], 15)
    assert ix._ranges_for([["d2", "d1", "d2", "nope", "d1"], ["d3", "d3"]]) == \
        ([(20, 30), (10, 20), (30, 40)], [0, 2, 3], 20)                  # first-mention order is kept
    assert ix._ranges_for([None])[2] == 45


def test_flat_search_with_a_repeated_document_equals_the_plain_filter():
    ix, X = _flat()
    for dup, plain in (([["d1", "d1"]], [["d1"]]), ([["d1", "d3", "d1"]], [["d1", "d3"]])):
        s, r = ix.search(X[[12]], 8, -1.0, dup)
        s0, r0 = ix.search(X[[12]], 8, -1.0, plain)
        assert torch.equal(r, r0) and torch.equal(s, s0)
        live = r[0][r[0] >= 0].tolist()
        assert len(set(live)) == len(live) == 8 and live[0] == 12
