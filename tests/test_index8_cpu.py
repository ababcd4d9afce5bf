"""fp8 (e4m3) flat vector index on the CPU reference (INDEX_DTYPE=fp8): the quantiser, the equivalence
with a bf16 index over the dequantised rows, the quality condition against the unquantised rows,
snapshots in all four combinations, WAL recovery, accounting, startup checks and an engine run."""
import numpy as np
import pytest
import torch

from docagents_amd import config
from docagents_amd.index import make_index
from docagents_amd.index.flat import FlatIndex, bytes_per_row, rows_for_budget
from docagents_amd.index.snapshot import load_index, save_index, snapshot_meta
from docagents_amd.index.wal import ShardLog
from docagents_amd.ops import reference as R
from docagents_amd.parallel import hbm_plan

BF16 = torch.bfloat16


def _unit(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=-1)


def _deq(ix):
    """The bf16 matrix an fp8 index stands for."""
    return R.index_dequant(ix.codes[:ix.n], ix.scale)


def test_quantiser_matches_quant_weight_fp8_pow2_and_dequantises_exactly():
    d = 96
    x = _unit(300, d, 1)
    x[7] = 0.0                      # all-zero row: scale 1
    x[8] = x[8] * 1e-3              # small rows get a small scale
    x[9, 0] = 448.0 * 2.0 ** -9     # amax exactly on a 448 * 2^e boundary
    x[9, 1:] *= 0.1
    ix = FlatIndex(d, "cpu", capacity=64, dtype="fp8")
    ix.add("a", np.arange(100), x[:100])          # grows past the capacity of 64
    ix.add_bulk(["b", "c"], [120, 80], np.arange(100, 300), x[100:])
    assert ix.dtype == "fp8" and not hasattr(ix, "X") and ix.codes.dtype == torch.uint8
    q, s = R.quant_weight_fp8_pow2(x.to(BF16))
    assert torch.equal(ix.codes[:300], q.view(torch.uint8)) and torch.equal(ix.scale[:300], s)
    assert float(ix.scale[7]) == 1.0 and not bool(ix.codes[7].any())
    assert float(ix.scale[9]) == 2.0 ** -9 and int(ix.codes[9, 0]) == 0x7E  # 448 = the largest e4m3
    # powers of two, and codes * scale is exact in bf16
    assert torch.equal(torch.exp2(torch.log2(s).round()), s)
    deq32 = q.float() * s[:, None]
    assert torch.equal(deq32.to(BF16).float(), deq32)
    assert torch.equal(ix.state_dict()["X"], deq32.to(BF16)) and ix.state_dict()["dtype"] == "fp8"
    assert FlatIndex(d, "cpu").state_dict()["dtype"] == "bf16"
    with pytest.raises(ValueError, match="dtype"):
        FlatIndex(d, "cpu", dtype="int8")


def _build_pair(d=64, cap=64):
    """An fp8 index driven through add / add_bulk / growth / removals, and a bf16 index given the
    dequantised rows through the same calls."""
    x = _unit(525, d, 2)
    x8 = FlatIndex(d, "cpu", capacity=cap, dtype="fp8")
    x16 = FlatIndex(d, "cpu", capacity=cap)
    xd = R.quant_weight_fp8_pow2(x.to(BF16))
    xd = (xd[0].float() * xd[1][:, None]).to(BF16)
    for ix, rows in ((x8, x), (x16, xd)):
        ix.add("d0", np.arange(40), rows[:40])
        ix.add("d1", np.arange(40, 100), rows[40:100])            # growth past 64
        ix.add_bulk(["d2", "d3", "d4"], [150, 120, 130], np.arange(100, 500), rows[100:500])
        ix.add("d0", np.arange(500, 520), rows[500:520])          # a second range of d0
        ix.add("d5", np.arange(520, 525), rows[520:525])
        assert ix.remove_doc("d3") == 120
        assert ix.remove_keys("d2", [105, 106, 180, 249]) == 4    # splits d2's range in four
        assert ix.remove_keys("d0", [0, 519]) == 2
    return x8, x16, x


def test_fp8_index_equals_bf16_index_over_the_dequantised_rows():
    x8, x16, x = _build_pair()
    assert len(x8.docs["d2"].ranges) == 3 and x8.docs["d2"].ranges == x16.docs["d2"].ranges
    assert torch.equal(_deq(x8), x16.X[:x16.n])
    q = torch.cat([x[[3, 60, 130, 300, 505]], _unit(4, 64, 5)])
    Q = q.shape[0]
    every = [f"d{i}" for i in range(5)]
    cases = [
        (10, -1.0, None),                                          # unfiltered dense scan
        (5, 0.3, None),                                            # with a floor
        (10, -1.0, [["d1"]] * Q),                                  # narrow filter: ranges
        (4, 0.2, [["d0"], ["d2", "d4"], ["d3"], ["nope"], None, ["d1"], ["d2"], ["d4"], ["d0", "d1"]]),
        (10, -1.0, [every] * Q),                                   # wide filter: bitmap
        (32, 0.1, [every[:3]] * Q),
        (32, -1.0, [["d1"]] * Q),                                  # k close to the 60 live rows
    ]
    wide = 0
    for k, thr, filt in cases:
        s8, i8 = x8.search(q, k, thr, filt)
        s16, i16 = x16.search(q, k, thr, filt)
        assert torch.equal(s8, s16) and torch.equal(i8, i16), (k, thr, filt)
        if filt is not None:
            wide += x8._ranges_for(filt)[2] * Q > 4 * x8.n
    assert wide >= 2, "no case took the bitmap path"
    # k larger than the live rows of the filter: padding after the live rows
    s8, i8 = x8.search(q[:2], 10, -1.0, [["d5"]] * 2)
    s16, i16 = x16.search(q[:2], 10, -1.0, [["d5"]] * 2)
    assert torch.equal(s8, s16) and torch.equal(i8, i16)
    assert sorted(i8[0, :5].tolist()) == list(range(520, 525)) and bool((i8[:, 5:] == -1).all())
    assert bool((s8[:, 5:] == float("-inf")).all())
    s8, i8 = FlatIndex(64, "cpu", dtype="fp8").search(q[:2], 3, -1.0)
    assert bool((i8 == -1).all())
    # removed rows never come back, and a row finds itself
    s, i = x8.search(x[130:131], 3, -1.0)
    assert int(i[0, 0]) == 130 and float(s[0, 0]) > 0.98
    s, i = x8.search(x[300:301], 32, -1.0)
    assert 300 not in i[0].tolist()  # d3 is gone
    ids8 = x8.search_ids(q, 5, -1.0)[1]
    assert torch.equal(ids8, x16.search_ids(q, 5, -1.0)[1])


@pytest.mark.parametrize("d,bound", [(384, 0.01), (768, 0.01), (1024, 0.01)])
def test_quality_condition_against_the_unquantised_rows(d, bound):
    """Unit-norm randn rows, N = 20000, 64 queries = rows + 0 / 0.5 / 1.0 x noise, seeds 1-3:
    quantising the rows moves no score by more than 0.01 and every query's own row stays top-1
    (measured with the reference: 0.0071 / 0.0062 / 0.0056 for d = 384 / 768 / 1024)."""
    N, worst = 20000, 0.0
    for seed in (1, 2, 3):
        g = torch.Generator().manual_seed(seed)
        X = torch.nn.functional.normalize(torch.randn(N, d, generator=g), dim=-1).to(BF16)
        own = torch.randperm(N, generator=g)[:64]
        lvl = torch.tensor([0.0, 0.5, 1.0]).repeat(22)[:64]
        noise = torch.nn.functional.normalize(torch.randn(64, d, generator=g), dim=-1)
        Qv = torch.nn.functional.normalize(X[own].float() + lvl[:, None] * noise, dim=-1).to(BF16)
        codes, scale = R.quant_weight_fp8_pow2(X)
        s16 = Qv.float() @ X.float().t()
        s8 = Qv.float() @ R.index_dequant(codes, scale).float().t()
        delta = float((s8 - s16).abs().max())
        worst = max(worst, delta)
        print(f"d={d} seed={seed}: max |delta score| = {delta:.4f}")
        assert delta <= bound, (d, seed, delta)
        top = R.topk_dense8(codes, scale, Qv, 1, -1.0)[1][:, 0]
        assert torch.equal(top.long(), own), (d, seed)
    print(f"d={d}: worst max |delta score| = {worst:.4f}")


@pytest.mark.parametrize("src,dst", [("fp8", "fp8"), ("fp8", "bf16"), ("bf16", "fp8"), ("bf16", "bf16")])
def test_snapshot_every_combination(tmp_path, src, dst):
    d = 64
    x = _unit(90, d, 7)
    a = FlatIndex(d, "cpu", dtype=src)
    a.add("p", np.arange(30), x[:30])
    a.add("gone", np.arange(30, 50), x[30:50])
    a.add("q", np.arange(50, 90), x[50:])
    a.remove_doc("gone")
    path = save_index(a, str(tmp_path / "s.safetensors"), durable=False)
    meta = snapshot_meta(path)
    assert meta.get("dtype", "bf16") == src and ("dtype" in meta) == (src == "fp8")
    from safetensors.torch import load_file
    t = load_file(path)
    assert set(t) == ({"codes", "scale", "ids"} if src == "fp8" else {"X", "ids"})
    if src == "fp8":
        assert t["codes"].dtype == torch.uint8 and t["codes"].shape == (70, d) and t["scale"].shape == (70,)
    b = FlatIndex(d, "cpu", dtype=dst)
    assert load_index(b, path) == 70
    live = torch.cat([x[:30], x[50:]]).to(BF16)
    q8, s8 = R.quant_weight_fp8_pow2(live)
    deq = (q8.float() * s8[:, None]).to(BF16)
    if src == "bf16" and dst == "bf16":
        assert torch.equal(b.X[:70], live)
    elif dst == "bf16":
        assert torch.equal(b.X[:70], deq)            # fp8 -> bf16 dequantises, exactly
    else:
        assert torch.equal(b.codes[:70], q8.view(torch.uint8)) and torch.equal(b.scale[:70], s8)
    sa, ia = a.search_ids(x[55:58], 5, -1.0, [["p", "q"]] * 3)
    sb, ib = b.search_ids(x[55:58], 5, -1.0, [["p", "q"]] * 3)
    assert torch.equal(ia, ib) and ib[:, 0].tolist() == [55, 56, 57]
    if src == dst or src == "fp8":
        assert torch.equal(sa, sb)


def test_wal_recovery_rebuilds_identical_codes(tmp_path):
    d = 64
    idx = FlatIndex(d, "cpu", dtype="fp8")
    log = ShardLog(str(tmp_path), fsync=False)
    assert log.recover(idx)["rows"] == 0
    log.put(idx, "a", np.arange(20), _unit(20, d, 1))          # fp32 in: the log keeps bf16
    log.put(idx, "b", np.arange(20, 50), _unit(30, d, 2))
    log.checkpoint(idx)                                        # an fp8 snapshot
    log.put(idx, "c", np.arange(50, 60), _unit(10, d, 3))
    log.remove(idx, "a")
    log.upsert(idx, "b", np.r_[45:50, 100:105], _unit(10, d, 4))  # replaces 5 chunks, adds 5
    log.close()                                                # "crash": nothing else is written
    idx2 = FlatIndex(d, "cpu", dtype="fp8")
    rec = ShardLog(str(tmp_path), fsync=False).recover(idx2)
    assert rec["snapshot_rows"] == 50 and rec["replayed"] == 3
    sel, _ = idx.live_rows_by_doc()
    sel2, docs2 = idx2.live_rows_by_doc()
    assert dict(docs2) == {"b": 35, "c": 10, "a": 0} or dict(docs2) == {"a": 0, "b": 35, "c": 10}
    by_id = {int(i): r for i, r in zip(idx.ids[sel], sel)}
    assert sorted(by_id) == sorted(int(i) for i in idx2.ids[sel2])
    for r2 in sel2:
        r = by_id[int(idx2.ids[r2])]
        assert torch.equal(idx2.codes[r2], idx.codes[r]) and idx2.scale[r2] == idx.scale[r]


def test_accounting():
    assert bytes_per_row(768) == bytes_per_row(768, "bf16") == 2 * 768 + 4
    assert bytes_per_row(768, "fp8") == 768 + 4
    assert rows_for_budget(768, 288) == int(288e9 // 1540) and rows_for_budget(768, 288, "fp8") == int(288e9 // 772)
    with pytest.raises(ValueError, match="dtype"):
        bytes_per_row(768, "int8")
    ix = FlatIndex(64, "cpu", dtype="fp8")
    ix.add("a", np.arange(10), _unit(10, 64, 1))
    assert ix.nbytes() == 10 * (64 + 4)
    ix16 = FlatIndex(64, "cpu")
    ix16.add("a", np.arange(10), _unit(10, 64, 1))
    assert ix16.nbytes() == 10 * 64 * 2
    assert hbm_plan.index_bytes(1000, 1024) == hbm_plan.index_bytes(1000, 1024, "bf16") == 1000 * (2048 + 12)
    assert hbm_plan.index_bytes(1000, 1024, "fp8") == 1000 * (1024 + 4 + 12)
    with pytest.raises(ValueError, match="dtype"):
        hbm_plan.index_bytes(1, 1, "int8")
    # the 100M x 1024 shard: 205 GB in bf16 leaves no room for a decoder, fp8 does
    assert hbm_plan.index_bytes(100_000_000, 1024) > 200e9 > 2 * hbm_plan.index_bytes(100_000_000, 1024, "fp8") - 10e9


def test_index_dtype_startup_checks():
    assert config.load({}).validate_engine().index_dtype == "bf16"
    assert config.load({"INDEX_DTYPE": "fp8"}).validate_engine().index_dtype == "fp8"
    both = config.load({"INDEX_DTYPE": "fp8", "KV_CACHE_DTYPE": "fp8", "TP_SIZE": "1"}).validate_engine()
    assert both.index_dtype == both.kv_cache_dtype == "fp8"
    assert config.load({"INDEX_DTYPE": "fp8", "TP_SIZE": "2"}).validate_engine().tp_size == 2  # no TP restriction
    with pytest.raises(ValueError, match="INDEX_DTYPE"):
        config.load({"INDEX_DTYPE": "int8"}).validate_engine()
    with pytest.raises(ValueError, match="INDEX_DTYPE"):
        config.load({"INDEX_DTYPE": "fp8", "INDEX_KIND": "ivfflat"}).validate_engine()
    assert make_index("flat", 64, "cpu", dtype="fp8").dtype == "fp8"
    assert make_index("flat", 64, "cpu").dtype == "bf16" and make_index("ivfflat", 64, "cpu").dtype == "bf16"
    with pytest.raises(ValueError, match="INDEX_DTYPE"):
        make_index("ivfflat", 64, "cpu", dtype="fp8")
    with pytest.raises(ValueError, match="INDEX_DTYPE"):
        make_index("flat", 64, "cpu", dtype="fp4")


def engine_smoke(device, tol):
    """A tiny-enc engine with an fp8 index ingests a few documents and every chunk's own text is
    searched. The randomly initialised tiny encoder maps every text to nearly the same vector (cosine
    0.9998-0.9999 between any two chunks, less than bf16 rounding of the vectors alone moves a score),
    so "own chunk first" holds for no index, bf16 included; what is asserted instead: the index holds
    exactly the quantised embeddings, every search equals the search of the dequantised bf16 rows
    (within ``tol``: 0 on the CPU, the GPU scans' 1e-4), and no score is more than the quality bound
    (0.01) away from the score of the unquantised bf16 embedding. Own-row top-1 on separable vectors
    is test_quality_condition_against_the_unquantised_rows."""
    from docagents_amd.engine.engine import Engine
    eng = Engine("tiny-enc", "tiny-dec", device, load_llm=False, use_graphs=False, index_dtype="fp8")
    assert eng.index.dtype == "fp8" and eng.index.kind == "flat" and eng.dim == 128
    docs = {"hbm": ["The MI355X carries 288 GB of HBM3E memory.", "Eight XCDs share the Infinity Fabric."],
            "rag": ["Chunks are embedded and stored in the flat index.", "A question retrieves its nearest chunks.",
                    "The decoder answers from the retrieved context."],
            "misc": ["Bananas are yellow and rich in potassium."]}
    cid = 0
    texts, vecs = [], []
    for doc, chunks in docs.items():
        v = eng.embed(chunks)
        eng.index.add(doc, np.arange(cid, cid + len(chunks)), v)
        texts += chunks
        vecs.append(v.cpu())
        cid += len(chunks)
    n = len(texts)
    q8, s8 = R.quant_weight_fp8_pow2(torch.cat(vecs).to(BF16))
    assert torch.equal(eng.index.codes[:n].cpu(), q8.view(torch.uint8)) and torch.equal(eng.index.scale[:n].cpu(), s8)
    qv = eng.embed(texts)
    ref = qv.cpu().float() @ R.index_dequant(q8, s8).float().t()   # [query, chunk]
    ref16 = qv.cpu().float() @ torch.cat(vecs).to(BF16).float().t()  # the unquantised bf16 rows
    for filt, live in ((None, range(n)), ([["rag"]] * n, (2, 3, 4))):
        s, ids = eng.index.search_ids(qv, n, 0.0, filt)
        s, ids = s.cpu(), ids.cpu()
        for i in range(n):
            got = [j for j in ids[i].tolist() if j >= 0]
            assert sorted(got) == list(live), (i, got)
            want = ref[i, got]
            assert float((s[i, :len(got)] - want).abs().max()) <= tol, (i, s[i], want)
            assert bool((s[i, :len(got) - 1] >= s[i, 1:len(got)]).all())
            # the quality condition on the engine's own vectors: no score moved by more than 0.01
            assert float((s[i, :len(got)] - ref16[i, got]).abs().max()) <= 0.01 + tol
            assert float(s[i, 0]) > 0.98
    return eng


def test_engine_with_fp8_index_searches_own_chunks():
    engine_smoke("cpu", 0.0)
