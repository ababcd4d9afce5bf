"""Engine / model / index behaviour on CPU (the fp32 reference op path) with tiny configs:
encoder normalisation, generation bookkeeping, map-reduce summarisation, index semantics
(filters, threshold, removal, snapshot), IVF recall and the engine RPC server with micro-batching."""
import asyncio
import socket

import numpy as np
import pytest
import torch

from docagents_amd.engine.engine import Engine
from docagents_amd.index.flat import FlatIndex
from docagents_amd.index.ivf import IVFFlatIndex
from docagents_amd.index.snapshot import load_index, save_index


@pytest.fixture(scope="module")
def eng():
    return Engine("tiny-enc", "tiny-dec", "cpu", max_batch=4, max_seq=512, max_new_tokens=6, summary_max_new=6,
                  use_graphs=False)


def test_embed_unit_norm_and_one_to_one(eng):
    v = eng.embed(["hello world", "", "  \x00 ", "Document: a.txt\n\nbody"])
    assert v.shape == (4, eng.dim)
    assert torch.allclose(v.float().norm(dim=-1), torch.ones(4), atol=1e-2)
    with pytest.raises(ValueError):
        eng.embed_one("  \x01  ")


def test_generation_confidence_and_lengths(eng):
    out = eng.answer_many([("q?", [[10, 11, 12] * 30], 0.8), ("q2?", [], 0.0)], 6)
    assert len(out) == 2
    (a1, c1), (a2, c2) = out
    assert 0 < c1 <= 0.8 and c2 == 0.0
    r = eng.gen.generate([[5, 6, 7], [8] * 40], 6)
    assert all(len(x.tokens) <= 6 and x.n_tokens >= 1 for x in r)


def test_summarize_map_reduce_long_input(eng):
    long_text = "alpha beta gamma delta " * 400  # > the tiny decoder's 512-token context
    s = eng.summarize_many([long_text, "short text"])
    assert len(s) == 2 and all(isinstance(x[0], str) and isinstance(x[1], list) for x in s)


def test_summarize_reduce_is_recursive_and_never_truncates():
    """A document of > 40 context windows (VERDICT r4 Next #2): every window's summary reaches a
    reduce prompt whole, the reduce runs more than one level (its summaries do not fit one context),
    no prompt exceeds the context, and each level's summaries reach the next level's prompts."""
    from docagents_amd.text.synthetic import TextGen
    e = Engine("tiny-enc", "tiny-dec", "cpu", max_batch=16, max_seq=512, max_new_tokens=4, summary_max_new=48,
               temperature=0.0, use_graphs=False)
    _, _, budget = e._summary_frame(48)
    doc = TextGen(seed=3).document(13000)
    n_win = -(-len(e._ids(doc)) // budget)
    assert n_win > 40
    calls = []
    orig = e.gen.generate

    def spy(prompts, max_new):
        r = orig(prompts, max_new)
        calls.append((prompts, e.chat.decode_many([x.tokens for x in r])))
        return r
    e.gen.generate = spy
    (summary, _), (short, _) = e.summarize_many([doc, "a short text"])
    assert len(calls) >= 3, [len(p) for p, _ in calls]  # map + at least two reduce levels
    assert all(len(p) + 48 <= 512 for ps, _ in calls for p in ps)

    def key(ids):
        return "," + ",".join(map(str, ids)) + ","
    for lvl in range(len(calls) - 1):
        prompts, outs = calls[lvl]
        if lvl == 0:
            outs = [o for o, p in zip(outs, prompts) if len(p) > 100][:n_win]  # the document's windows
        nxt = [key(p) for p in calls[lvl + 1][0]]
        for o in outs:
            ids = e._ids(o)
            assert not ids or any(key(ids) in p for p in nxt), (lvl, o[:80])
    assert len(calls[-1][0]) == 1  # the last level is one prompt: the final summary


def test_summarize_reduce_converges_with_a_large_max_new():
    """with max_new above ~max_seq / 3 a generated summary no longer fits half a reduce
    prompt, and each level used to yield as many prompts as the last until the 64-level guard. The
    reduce levels now generate with the largest budget that converges; the map windows keep max_new."""
    from docagents_amd.text.synthetic import TextGen
    e = Engine("tiny-enc", "tiny-dec", "cpu", max_batch=16, max_seq=512, max_new_tokens=4, summary_max_new=300,
               temperature=0.0, use_graphs=False)
    doc = TextGen(seed=5).document(3000)
    news = []
    orig = e.gen.generate

    def spy(prompts, max_new):
        news.append((len(prompts), max_new))
        assert all(len(p) + max_new <= 512 for p in prompts)
        return orig(prompts, max_new)
    e.gen.generate = spy
    (summary, _), = e.summarize_many([doc])
    assert news[0][1] == 300 and len(news) >= 2, news   # map windows at max_new, then reduce levels
    assert all(n < 300 for _, n in news[1:]) and news[-1][0] == 1, news
    assert e.stats["summary_reduce_levels_max"] < 64


def _unit(n, d, seed=0):
    x = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    return torch.from_numpy(x / np.linalg.norm(x, axis=1, keepdims=True))


def test_flat_index_filters_threshold_removal_snapshot(tmp_path):
    X = _unit(40, 32)
    ix = FlatIndex(32, "cpu")
    for i in range(4):
        ix.add(f"d{i}", np.arange(10 * i, 10 * i + 10) + 1000, X[10 * i:10 * i + 10])
    s, r = ix.search(X[[3, 25]], 3, -1.0, [["d0"], ["d2", "d3"]])
    assert int(ix.row_ids(r[0].numpy())[0]) == 1003 and int(ix.row_ids(r[1].numpy())[0]) == 1025
    s, r = ix.search(X[[3]], 5, 0.99, [["d0", "d1"]])  # only the self-match passes the floor
    assert (r[0] >= 0).sum() == 1
    assert ix.remove_doc("d0") == 10
    s, r = ix.search(X[[3]], 3, -1.0, None)
    assert all(int(x) >= 10 for x in r[0] if x >= 0)
    p = save_index(ix, str(tmp_path / "shard0.safetensors"))
    ix2 = FlatIndex(32, "cpu")
    assert load_index(ix2, p) == 30
    s2, r2 = ix2.search(X[[25]], 3, -1.0, [["d2"]])
    assert int(ix2.row_ids(r2[0].numpy())[0]) == 1025


def test_ivf_recall_and_delta_rows():
    rng = np.random.default_rng(2)
    centers = rng.standard_normal((10, 48)).astype(np.float32)
    lab = rng.integers(0, 10, 2000)
    X = centers[lab] + 0.2 * rng.standard_normal((2000, 48)).astype(np.float32)
    X = torch.from_numpy(X / np.linalg.norm(X, axis=1, keepdims=True))
    ix = IVFFlatIndex(48, "cpu", lists=10, probes=3)
    for i in range(0, 1800, 100):
        ix.add(f"d{i}", np.arange(i, i + 100), X[i:i + 100])
    assert ix.train(iters=6)
    ix.add("late", np.arange(1800, 2000), X[1800:])  # delta region, scanned exactly
    Q = X[rng.choice(2000, 30, replace=False)]
    s, r = ix.search(Q, 5, -1.0, None)
    # rows are list-major after training: compare external ids
    rec = np.mean([len(set(np.argsort(-(X @ Q[i]).numpy())[:5]) & set(ix.row_ids(r[i].numpy()).tolist())) / 5
                   for i in range(30)])
    assert rec > 0.8
    s, r = ix.search(X[[1900]], 1, -1.0, [["late"]])
    assert int(ix.row_ids(r[0].numpy())[0]) == 1900
    assert ix.remove_doc("d0") == 100
    s, r = ix.search(X[:100], 5, -1.0, None)
    assert all(i >= 100 for i in ix.row_ids(r.numpy().ravel()) if i >= 0)  # removed rows never match
    rows, docs = ix.live_rows_by_doc()
    assert len(rows) == 1900 and dict(docs)["late"] == 200 and "d0" not in dict(docs)


def test_ivf_streaming_build_matches_exact_search():
    dim, n = 64, 6000
    cent = torch.nn.functional.normalize(torch.randn(40, dim, generator=torch.Generator().manual_seed(0)), dim=-1)

    def gen(c, rows=1000):
        g = torch.Generator().manual_seed(100 + c)
        lab = torch.randint(0, 40, (rows,), generator=g)
        x = cent[lab] + 0.15 * torch.randn(rows, dim, generator=g)
        return torch.nn.functional.normalize(x, dim=-1).to(torch.bfloat16)

    ix = IVFFlatIndex(dim, "cpu", lists=40, probes=6).build_streaming(gen, n, 1000, rows_per_doc=50, iters=5,
                                                                      sample=4000)
    assert len(ix) == n and int(ix.list_off[-1]) == n
    Xall = torch.cat([gen(c) for c in range(6)]).float()
    Q = Xall[torch.arange(0, n, 97)]
    s, r = ix.search(Q, 10, -1.0, None)
    rec = np.mean([len(set(torch.topk(Xall @ Q[i], 10).indices.tolist()) & set(ix.row_ids(r[i].numpy()).tolist()))
                   / 10 for i in range(Q.shape[0])])
    assert rec > 0.9, rec
    s, r = ix.search(Q[:3], 5, -1.0, [["d7"]] * 3)  # doc filter: rows 350..399
    ids = ix.row_ids(r.numpy().ravel())
    assert all(350 <= i < 400 for i in ids if i >= 0) and (ids >= 0).sum() == 15


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_engine_rpc_server_microbatching(eng):
    from docagents_amd.engine.rpc import EngineClient
    from docagents_amd.engine.server import EngineGroup, EngineServer
    from docagents_amd.providers import RemoteEmbedder, RemoteLLM
    from docagents_amd.store.vectors import EngineVectors
    from docagents_amd.utils.log import discard

    async def go():
        srv = EngineServer(EngineGroup(eng), discard())
        port = _port()
        await srv.start(f"tcp://127.0.0.1:{port}")
        cl = await EngineClient(f"tcp://127.0.0.1:{port}").connect()
        emb, llm, vec = RemoteEmbedder(cl), RemoteLLM(cl), EngineVectors(cl)
        # 8 concurrent single-text embeds -> coalesced into fewer encoder batches
        outs = await asyncio.gather(*[emb.embed(f"question {i}") for i in range(8)])
        assert all(o.shape == (eng.dim,) for o in outs)
        assert srv.stats["embed_raw"]["batches"] < 8
        vs = await emb.embed_batch(["a b", "c d", ""])
        assert len(vs) == 3
        u = _unit(3, eng.dim, 5).numpy()
        await vec.add("docX", np.array([7, 8, 9]), u)
        hits = await vec.search(u[1], ["docX"], 2, -1.0)
        assert hits[0][0] == 8
        s, kp = await llm.summarize("some text to summarize")
        a, c = await llm.answer("q?", "ctx text", 0.5)
        a2, c2 = await llm.answer_chunks("q?", [("ctx", [5, 6, 7]), ("other", None)], 0.5)
        assert isinstance(s, str) and isinstance(kp, list) and 0 <= c <= 0.5 and 0 <= c2 <= 0.5
        st = await cl.call("stats")
        assert st["ranks"][0]["index_rows"] >= 3
        await cl.close()
        srv.server.close()
    asyncio.run(go())


def test_engine_health_and_metrics(eng):
    from prometheus_client import generate_latest

    from docagents_amd.engine.rpc import EngineClient
    from docagents_amd.engine.server import EngineGroup, EngineServer
    from docagents_amd.utils.log import discard

    async def go():
        srv = EngineServer(EngineGroup(eng), discard())
        port = _port()
        await srv.start(f"tcp://127.0.0.1:{port}")
        cl = await EngineClient(f"tcp://127.0.0.1:{port}").connect()
        await cl.call("embed", texts=["x y z"], preprocess=True)
        await cl.call("answer", items=[{"question": "q?", "context": "c", "quality": 1.0}])
        st = await cl.call("stats")
        h = await cl.call("health")
        # answer + stats ran on the GPU thread; the query-sized embed on the fast lane
        assert h["ok"] is True and h["steps"] >= 2 and h["world"] == 1 and h["search_plane"] is True
        assert st["batching"]["embed_fast"]["items"] == 1
        await cl.close()
        srv.server.close()
    asyncio.run(go())
    text = generate_latest().decode()
    for name in ("da_engine_step_seconds", "da_engine_batches_total", "da_engine_tokens_total",
                 "da_engine_index_rows"):
        assert name in text, name


def test_watchdog_flags_and_recovers():
    from docagents_amd.engine.observe import Watchdog
    hard = []
    w = Watchdog(soft_s=5.0, hard_s=10.0, on_hard=lambda c, e: hard.append(c))
    w.begin("answer")
    t0 = w._cur[1]
    w.check(t0 + 1.0)
    assert w.healthy
    w.check(t0 + 6.0)
    assert not w.healthy and w.state()["stuck"] == "answer" and not hard
    w.check(t0 + 11.0)
    assert hard == ["answer"]
    w.end()
    assert w.healthy and w.steps == 1


def test_unhealthy_engine_fails_fast(eng):
    from docagents_amd.engine.server import EngineGroup, EngineServer
    from docagents_amd.utils.log import discard

    async def go():
        srv = EngineServer(EngineGroup(eng), discard())
        srv.watchdog.stuck = "answer"
        try:
            await srv._gpu("embed", {"texts": ["a"]})
        except RuntimeError as e:
            assert "unhealthy" in str(e)
        else:
            raise AssertionError("expected fail-fast")
        assert (await srv._gpu("ping", {})) == [0]
    asyncio.run(go())


def test_step_profiler_writes_trace(tmp_path):
    from docagents_amd.engine.observe import StepProfiler
    p = StepProfiler(f"{tmp_path}:1")
    import torch
    assert p.run("embed", lambda a: torch.ones(8).sum() + a, 1) == 9
    assert not p.active
    files = sorted(x.name for x in tmp_path.iterdir())
    assert files == ["rank0_001_embed.json", "rank0_001_embed.txt"]
    assert p.run("embed", lambda: 3) == 3  # exhausted -> passthrough


def test_continuous_batching_matches_waves_greedy():
    from docagents_amd.engine.generator import ContinuousScheduler
    e = Engine("tiny-enc", "tiny-dec", "cpu", max_batch=4, max_seq=256, max_new_tokens=6, temperature=0.0,
               use_graphs=False)
    rng = np.random.default_rng(1)
    prompts = [list(rng.integers(5, 3000, size=n)) for n in (7, 30, 3, 12, 50, 9)]
    budgets = [3, 6, 1, 5, 2, 6]
    want = [e.gen.generate([p], b)[0].tokens for p, b in zip(prompts, budgets)]
    sched = ContinuousScheduler(e.gen, B=4, max_new_cap=8, chunk_steps=2)
    got = {}
    for i in range(2):
        sched.submit(prompts[i], budgets[i], i)
    for tag, r in sched.tick():
        got[tag] = r.tokens
    for i in range(2, 6):  # arrive mid-generation; more requests than rows -> queueing
        sched.submit(prompts[i], budgets[i], i)
    while sched.busy():
        for tag, r in sched.tick():
            got[tag] = r.tokens
    assert [got[i] for i in range(6)] == want
    assert [len(t) for t in want] == budgets
    assert sched.stats["admitted"] == sched.stats["finished"] == 6
    assert len(e.gen.cache.free) == e.gen.cache.slots - 1  # only the dummy slot stays taken


def test_engine_server_continuous_batching(eng):
    from docagents_amd.engine.rpc import EngineClient
    from docagents_amd.engine.server import EngineGroup, EngineServer
    from docagents_amd.providers import RemoteLLM
    from docagents_amd.utils.log import discard

    async def go():
        srv = EngineServer(EngineGroup(eng), discard(), continuous=True, cb_steps=2)
        port = _port()
        await srv.start(f"tcp://127.0.0.1:{port}")
        cl = await EngineClient(f"tcp://127.0.0.1:{port}").connect()
        llm = RemoteLLM(cl)
        # 7 concurrent answers through a 4-row scheduler, plus an embed interleaved between ticks
        outs = await asyncio.gather(*[llm.answer(f"question {i}?", "context words " * (i + 1), 0.5) for i in range(7)],
                                    cl.call("embed", texts=["x"], preprocess=True))
        answers = outs[:7]
        assert all(isinstance(a, str) and 0 <= c <= 0.5 for a, c in answers)
        st = srv.stats["answer_cb"]
        assert st["items"] == 7 and st["ticks"] >= 2
        assert eng.scheduler.stats["finished"] >= 7 and not eng.scheduler.busy()
        await cl.close()
        srv.server.close()
    asyncio.run(go())


def test_continuous_summaries_match_wave_summaries():
    """Summaries through the continuous scheduler (map windows + reduce for a text longer than the
    context) give the same text as the whole-batch path, with answers decoding alongside."""
    from docagents_amd.engine.rpc import EngineClient
    from docagents_amd.engine.server import EngineGroup, EngineServer
    from docagents_amd.providers import RemoteLLM
    from docagents_amd.utils.log import discard
    e = Engine("tiny-enc", "tiny-dec", "cpu", max_batch=4, max_seq=512, max_new_tokens=5, summary_max_new=6,
               temperature=0.0, use_graphs=False)
    texts = ["alpha beta gamma " * 5, "delta epsilon " * 3, "word " * 1200, "zeta eta theta iota"]
    want = e.summarize_many(texts)
    wins, owner = e.summary_windows(texts)
    assert sum(1 for i, part in owner if part and i == 2) >= 2  # the long text is map-reduced

    async def go():
        srv = EngineServer(EngineGroup(e), discard(), continuous=True, cb_steps=2)
        port = _port()
        await srv.start(f"tcp://127.0.0.1:{port}")
        cl = await EngineClient(f"tcp://127.0.0.1:{port}").connect()
        llm = RemoteLLM(cl)
        outs = await asyncio.gather(*[llm.summarize(t) for t in texts],
                                    *[llm.answer(f"q{i}?", "ctx " * (i + 2), 1.0) for i in range(3)])
        await cl.close()
        srv.server.close()
        return outs[:len(texts)]
    got = asyncio.run(go())
    assert [(s, list(kp)) for s, kp in got] == [(s, list(kp)) for s, kp in want]
    # every slot is back except the dummy and the cached prompt heads
    assert not e.scheduler.busy() and len(e.gen.cache.free) == (e.gen.cache.slots - 1 - len(e.scheduler.heads)
                                                                  - (e.gen.head is not None))


def test_engine_search_microbatch_matches_single_searches(eng):
    """Concurrent searches (mixed document filters, one without) coalesce into fewer index scans
    and return exactly what each search returns alone."""
    from docagents_amd.engine.rpc import EngineClient
    from docagents_amd.engine.server import EngineGroup, EngineServer
    from docagents_amd.utils.log import discard

    async def go():
        srv = EngineServer(EngineGroup(eng), discard())
        port = _port()
        await srv.start(f"tcp://127.0.0.1:{port}")
        cl = await EngineClient(f"tcp://127.0.0.1:{port}").connect()
        u = _unit(24, eng.dim, 11).numpy()
        for j, d in enumerate(("sA", "sB", "sC")):
            await cl.call("index_add", doc_id=d, keys=np.arange(100 * j, 100 * j + 8), vecs=u[8 * j:8 * j + 8])
        qs = _unit(9, eng.dim, 12).numpy()
        flt = [["sA"], ["sB", "sC"], None, ["sC"], ["sA", "sB", "sC"], ["sB"], None, ["sA"], ["sC"]]
        args = [dict(vecs=qs[i:i + 1], filters=None if f is None else [f], k=3, min_sim=-1.0)
                for i, f in enumerate(flt)]
        alone = [await cl.call("search", **a) for a in args]
        b0 = srv.group.plane.stats["scans"]
        together = await asyncio.gather(*[cl.call("search", **a) for a in args])
        assert srv.group.plane.stats["scans"] - b0 < len(args)  # coalesced into shared scans
        for x, y in zip(alone, together):
            assert np.array_equal(x["keys"], y["keys"]) and np.allclose(x["scores"], y["scores"])
        # a malformed search fails alone; the batcher keeps serving
        try:
            await cl.call("search", vecs=np.zeros((1, 7), dtype=np.float32), filters=None, k=3, min_sim=-1.0)
        except Exception as e:  # noqa: BLE001
            assert "reshape" in str(e) or "size" in str(e)
        else:
            raise AssertionError("expected a shape error")
        again = await cl.call("search", **args[0])
        assert np.array_equal(again["keys"], alone[0]["keys"])
        await cl.close()
        srv.server.close()
    asyncio.run(go())


def test_config_bool_parsing():
    from docagents_amd.config import load
    assert load({"ENGINE_CONTINUOUS": "false"}).engine_continuous is False
    assert load({"ENGINE_CONTINUOUS": "1"}).engine_continuous is True
    assert load({"ENGINE_CONTINUOUS": "maybe"}).engine_continuous is True  # parse error -> default


def test_encoder_fp8_close_to_bf16_reference_path():
    from docagents_amd.models.bert import BertEncoder
    from docagents_amd.models.configs import encoder_config
    cfg = encoder_config("tiny-enc")
    a = BertEncoder(cfg, "cpu", seed=3)
    b = BertEncoder(cfg, "cpu", weights=a.w, dtype="fp8")
    seqs = [[101, 7, 8, 9, 102], [101] + list(range(200, 260)) + [102]]
    va, vb = a.encode_packed(seqs), b.encode_packed(seqs)
    cos = (va * vb).sum(-1)
    assert torch.all(cos > 0.98), cos


def test_shared_prompt_head_prefilled_once_same_tokens():
    """Prompts sharing a long head (the Answer system prompt): the head is prefilled once, the
    suffixes attend to it from the cache, and the generations equal the unshared path's."""
    e = Engine("tiny-enc", "tiny-dec", "cpu", max_batch=4, max_seq=512, max_new_tokens=6, temperature=0.0,
               use_graphs=False)
    rng = np.random.default_rng(7)
    head = list(rng.integers(5, 3000, size=130))
    prompts = [head + list(rng.integers(5, 3000, size=n)) for n in (1, 17, 40, 5)]
    g = e.gen
    assert g.shared_prefix_len(prompts) == 128  # rounded down to the 64-key decode tile
    assert g.shared_prefix_len(prompts[:1]) == 0 and g.shared_prefix_len([head[:20] + [1], head[:20] + [2]]) == 0
    g.share_prefix = False
    want = g.generate(prompts, 6)
    t_plain = g.stats["prefill_tokens"]
    g.share_prefix = True
    got = g.generate(prompts, 6)
    assert [r.tokens for r in got] == [r.tokens for r in want]
    assert all(abs(a.mean_prob - b.mean_prob) < 1e-3 for a, b in zip(got, want))
    assert g.stats["shared_prefix_tokens"] == 128 * 3
    assert g.stats["prefill_tokens"] - t_plain == t_plain - 128 * 3
    # every slot back except the dummy and the kept head
    assert g.head is not None and g.head["P"] == 128
    assert len(g.cache.free) == g.cache.slots - 2
    # a later single prompt with the same head reuses the kept head (no head prefill), same tokens
    single = head + list(rng.integers(5, 3000, size=9))
    t0 = g.stats["prefill_tokens"]
    got1 = g.generate([single], 6)[0]
    assert g.stats["prefill_tokens"] - t0 == len(single) - 128 and g.stats["head_cache_hits"] == 1
    g.share_prefix = False  # the kept head is ignored while sharing is off
    ref1 = g.generate([single], 6)[0]
    g.share_prefix = True
    assert got1.tokens == ref1.tokens and abs(got1.mean_prob - ref1.mean_prob) < 1e-3


def test_continuous_batching_caches_prompt_head():
    """ContinuousScheduler keeps the head shared by an admission's prompts in a slot of its own;
    later prompts with that head (even alone) prefill only their suffix; generations equal the
    per-prompt greedy path; the head slot stays reserved, every row slot is returned."""
    from docagents_amd.engine.generator import ContinuousScheduler
    e = Engine("tiny-enc", "tiny-dec", "cpu", max_batch=4, max_seq=512, max_new_tokens=6, temperature=0.0,
               use_graphs=False)
    rng = np.random.default_rng(5)
    head = [int(t) for t in rng.integers(5, 3000, size=150)]
    prompts = [head + [int(t) for t in rng.integers(5, 3000, size=n)] for n in (3, 40, 11, 7, 25)]
    other = [int(t) for t in rng.integers(5, 3000, size=30)]
    e.gen.share_prefix = False
    want = [e.gen.generate([p], 5)[0].tokens for p in prompts + [other]]
    e.gen.share_prefix = True
    sched = ContinuousScheduler(e.gen, B=4, max_new_cap=8, chunk_steps=2)
    got = {}
    for i in range(3):
        sched.submit(prompts[i], 5, i)
    for tag, r in sched.tick():
        got[tag] = r.tokens
    assert sched.stats["heads_built"] == 1 and sched.heads[0]["P"] == 128
    for i in (3, 4):
        sched.submit(prompts[i], 5, i)
    sched.submit(other, 5, 5)
    while sched.busy():
        for tag, r in sched.tick():
            got[tag] = r.tokens
    assert [got[i] for i in range(6)] == want
    assert sched.stats["heads_built"] == 1 and sched.stats["head_hits"] == 5
    assert sched.heads[0]["refs"] == 0
    assert len(e.gen.cache.free) == e.gen.cache.slots - 2  # dummy slot + the cached head's slot


def test_interleaved_rope_conversion_preserves_attention_scores():
    """HF rotate_half checkpoints run on this engine's interleaved-pair RoPE (so the prefill QKV GEMM can
    rotate inside its epilogue) after to_interleaved_rope permutes the q / k rows of every head:
    q.k per head and the v rows are unchanged."""
    from docagents_amd.models.llama import to_interleaved_rope
    from docagents_amd.ops import reference as R
    torch.manual_seed(0)
    H, Hkv, D, hid, T = 4, 2, 96, 64, 9
    w = torch.randn((H + 2 * Hkv) * D, hid, dtype=torch.float64)
    x = torch.randn(T, hid, dtype=torch.float64)
    pos = torch.arange(T) * 7 + 3
    cs = R.rope_table(128, D, 10000.0).double()[pos]

    def rotate_half_rope(z):  # HF layout: pairs (i, i + D/2)
        z1, z2 = z[..., :D // 2], z[..., D // 2:]
        c, s = cs[:, None, :, 0], cs[:, None, :, 1]
        return torch.cat([z1 * c - z2 * s, z2 * c + z1 * s], dim=-1)

    def interleaved_rope(z):  # this engine: pairs (2i, 2i + 1)
        z1, z2 = z[..., 0::2], z[..., 1::2]
        c, s = cs[:, None, :, 0], cs[:, None, :, 1]
        return torch.stack([z1 * c - z2 * s, z2 * c + z1 * s], dim=-1).flatten(-2)

    def scores(qkv, rope):
        q = rope(qkv[:, :H * D].view(T, H, D))
        k = rope(qkv[:, H * D:(H + Hkv) * D].view(T, Hkv, D)).repeat_interleave(H // Hkv, 1)
        return torch.einsum("qhd,khd->hqk", q, k), qkv[:, (H + Hkv) * D:]

    s_hf, v_hf = scores(x @ w.t(), rotate_half_rope)
    s_il, v_il = scores(x @ to_interleaved_rope(w, H, Hkv, D).t(), interleaved_rope)
    torch.testing.assert_close(s_il, s_hf, rtol=1e-10, atol=1e-10)
    assert torch.equal(v_il, v_hf)
    # the fp32 reference kernel implements the interleaved layout
    qkv = (x @ to_interleaved_rope(w, H, Hkv, D).t()).float().to(torch.bfloat16)
    got = R.rope_cache(qkv.clone(), pos.int(), R.rope_table(128, D, 10000.0), H, Hkv, D)
    want = interleaved_rope(qkv.double()[:, :(H + Hkv) * D].view(T, H + Hkv, D)).reshape(T, -1)
    torch.testing.assert_close(got[:, :(H + Hkv) * D].double(), want, rtol=0.02, atol=0.02)


def test_batched_tokenization_matches_serial(eng):
    """summary windows / reduce prompts / answer tails are tokenized with encode_batch and
    detokenized with decode_batch: identical ids and texts to one call per string."""
    texts = ["alpha beta gamma " * 50, "", "delta <|end|> epsilon", "zeta\nêta " * 300]
    assert eng._ids_many(texts) == [eng._ids(t) for t in texts]
    seqs = [eng._ids(t) for t in texts]
    assert eng.chat.decode_many(seqs) == [eng.chat.decode(s) for s in seqs]
    w, owner = eng.summary_windows(texts, 16)
    head, tail, budget = eng._summary_frame(16)
    want = []
    for t in texts:
        ids = eng._ids(t)
        want.extend([head + ids + tail] if len(ids) <= budget else
                     [head + ids[s:s + budget] + tail for s in range(0, len(ids), budget)])
    assert w == want
    q = "what is alpha?"
    assert eng.answer_prompt_ids(q, [[5, 6]], 16) == \
        eng.answer_prompt_ids(q, [[5, 6]], 16, tail=eng._ids_many([eng._answer_tail(q)] * 2)[0])


def test_kept_head_slot_never_blocks_a_full_wave():
    """A Generator that allocates its own cache (max_batch + 1 slots) must not keep a prompt-head
    slot taken from a full wave's budget: 2 shared-head prompts, then max_batch prompts, both run
    (round-2 advisor finding, generator.py:76)."""
    from docagents_amd.engine.generator import Generator
    from docagents_amd.models.configs import decoder_config
    from docagents_amd.models.llama import LlamaDecoder
    m = LlamaDecoder(decoder_config("tiny-dec"), "cpu", seed=0)
    g = Generator(m, max_batch=4, max_seq=512, temperature=0.0, use_graphs=False)
    rng = np.random.default_rng(3)
    head = [int(t) for t in rng.integers(5, 3000, size=130)]
    two = [head + [int(t) for t in rng.integers(5, 3000, size=n)] for n in (3, 9)]
    assert len(g.generate(two, 4)) == 2
    full = [head + [int(t) for t in rng.integers(5, 3000, size=n)] for n in (1, 2, 3, 4)]
    assert len(g.generate(full, 4)) == 4
    assert len(g.cache.free) + 1 + (g.head is not None) == g.cache.slots


def test_continuous_scheduler_runs_the_smallest_row_bucket():
    """An unloaded request decodes in the 1-row bucket (batch-1 cost), three in the 4-row bucket;
    the tokens equal the wave path's either way."""
    from docagents_amd.engine.generator import ContinuousScheduler
    e = Engine("tiny-enc", "tiny-dec", "cpu", max_batch=8, max_seq=512, max_new_tokens=6, temperature=0.0,
               use_graphs=False)
    rng = np.random.default_rng(9)
    prompts = [[int(t) for t in rng.integers(5, 3000, size=n)] for n in (12, 40, 7)]
    e.gen.share_prefix = False
    want = [e.gen.generate([p], 6)[0].tokens for p in prompts]
    sched = ContinuousScheduler(e.gen, B=8, max_new_cap=8, chunk_steps=4)
    got1 = sched.run_all(prompts[:1], 6)
    assert got1[0].tokens == want[0] and set(sched.stats["steps_by_bucket"]) == {1}
    got3 = sched.run_all(prompts, 6)
    assert [r.tokens for r in got3] == want
    assert sched.stats["steps_by_bucket"].get(4, 0) > 0 and 8 not in sched.stats["steps_by_bucket"]


def test_dk_decode_step_matches_fused_norm_step(monkeypatch):
    """The gemm_dk decode layer structure (norms deferred into the consuming GEMM from per-part sums
    of squares, ops/reference.py gemm_dk) produces the same logits as the split-K + fused-norm
    structure it replaces for 2..32 rows, within bf16 rounding, step after step."""
    from docagents_amd.models.configs import decoder_config
    from docagents_amd.models.llama import DecodeState, LlamaDecoder
    from docagents_amd.ops import gemm_plan
    torch.manual_seed(0)
    m = LlamaDecoder(decoder_config("tiny-dec"), "cpu", seed=0)
    m.alloc_cache(6, 256)
    B = 4
    assert m._dk_decode(B)
    out = {}
    for dk in (True, False):
        monkeypatch.setattr(gemm_plan, "DECODE_DK", dk)  # the planner's switch: the CPU ops read it there
        assert m._dk_decode(B) == dk
        st = DecodeState(m, B, 8, 0.0, 0, ())
        st.slot.copy_(torch.arange(B, dtype=torch.int32))
        st.lens.fill_(1); st.pos.zero_(); st.active.fill_(1); st.start.zero_()
        st.tokens.copy_(torch.tensor([5, 77, 300, 1234], dtype=torch.int32))
        logits = []
        for _ in range(3):
            m.decode_step(st)
            logits.append(st.logits.float().clone())
        out[dk] = logits
    monkeypatch.undo()
    for a, b in zip(out[True], out[False]):
        assert torch.allclose(a, b, atol=0.05, rtol=0.02), (a - b).abs().max()


def test_fp16_encoder_matches_bf16_encoder_cpu():
    """DTYPE=fp16 (BASELINE config 4): the encoder on fp16 weights / activations gives the same unit
    vectors as the bf16 one to rounding (CPU reference ops; the kernels: tests/test_models_gpu.py)."""
    import copy

    from docagents_amd.models.bert import BertEncoder
    from docagents_amd.models.configs import encoder_config
    cfg = encoder_config("tiny-enc")
    a = BertEncoder(cfg, "cpu", seed=3)
    b = BertEncoder(cfg, "cpu", weights=copy.deepcopy(a.w), dtype="fp16")
    assert b.w["word"].dtype == torch.float16 and b.w["layers"][0]["wqkv"].dtype == torch.float16
    seqs = [[101, 2000 + i, 3000 + 2 * i, 102] for i in range(5)] + [list(range(100, 140))]
    va, vb = a.encode_packed(seqs), b.encode_packed(seqs)
    cos = (va.float() * vb.float()).sum(-1)
    assert cos.min() > 0.999, cos


def test_grouped_admission_rule(eng):
    """VERDICT r5 Next #4: under load, arrivals are admitted in groups (admit_min of them, or as
    many as there are free rows, or after admit_wait_s), not one prefill per arrival; at light load
    (< admit_hold_frac of the rows busy) an arrival is admitted at once."""
    import time as _t
    from types import SimpleNamespace

    from docagents_amd.engine.server import EngineGroup, EngineServer
    from docagents_amd.utils.log import discard
    srv = EngineServer(EngineGroup(eng), discard(), continuous=True, admit_min=4, admit_wait_s=0.2,
                       admit_hold_frac=0.25)
    fake = SimpleNamespace(n_active=0, B=16, pending=[])
    eng._sched = fake
    try:
        assert not srv._admit_ready()  # nothing waiting
        srv._cb_new, srv._cb_oldest = [(1, {})], _t.monotonic()
        assert srv._admit_ready()      # idle engine: latency first
        fake.n_active = 3
        assert srv._admit_ready()      # 3 < 0.25 * 16 busy: still light
        fake.n_active = 8
        assert not srv._admit_ready()  # loaded: hold for a group of 4
        srv._cb_new = [(i, {}) for i in range(4)]
        assert srv._admit_ready()
        srv._cb_new = [(1, {})]
        fake.n_active = 15
        assert srv._admit_ready()      # only one free row: a group of one is full
        fake.n_active = 16
        assert not srv._admit_ready()  # no free row: run until rows free up
        fake.n_active, srv._cb_oldest = 8, _t.monotonic() - 0.25
        assert srv._admit_ready()      # the oldest waited past admit_wait_s
        srv.admit_min = 1
        srv._cb_oldest = _t.monotonic()
        assert srv._admit_ready()      # ENGINE_ADMIT_MIN=1: every arrival at once
    finally:
        eng._sched = None


def test_scheduler_steps_to_free():
    e = Engine("tiny-enc", "tiny-dec", "cpu", max_batch=4, max_seq=256, max_new_tokens=6, temperature=0.0,
               use_graphs=False)
    sch = e.scheduler
    assert sch.steps_to_free() == 1
    sch.submit([5, 6, 7], 6, "a")
    sch.submit([5, 6, 8, 9], 3, "b")
    sch.tick(steps=1)
    assert sch.steps_to_free() == 1  # "b": budget 3, one token at prefill, one step run
    while sch.busy():
        sch.tick()


def test_auto_decode_batch_from_the_kv_budget():
    """ENGINE_MAX_BATCH=0 (the default): the largest power-of-two batch <= 128 whose KV cache
    (batch + 4 slots) fits KV_CACHE_GB, 64 on a CPU without a budget."""
    from docagents_amd.models.configs import decoder_config
    from docagents_amd.models.llama import KVCache
    e = Engine("tiny-enc", "tiny-dec", "cpu", max_batch=0, max_seq=256, max_new_tokens=4, use_graphs=False)
    assert e.gen.max_batch == 64
    per = KVCache.bytes_for(decoder_config("tiny-dec"), 1, 256)
    assert e.auto_batch(256, kv_gb=(36 * per) / 1e9) == 32          # 32 + 4 slots fit, 64 + 4 do not
    assert e.auto_batch(256, kv_gb=1e6) == Engine.AUTO_BATCH_MAX
    # MI355X: Phi-3-mini (7.6 GB of weights) leaves ~280 GB free -> 128 rows = 213 GB of KV within
    # 280 GB less the reserve; Llama-3-70B TP=1 (141 GB of weights) leaves room for 64 rows only
    free_phi, free_70b = 280e9, 288e9 - 141e9
    assert KVCache.bytes_for(decoder_config("phi3-mini"), 132, 4096) <= free_phi - Engine.AUTO_RESERVE_BYTES
    per70 = KVCache.bytes_for(decoder_config("llama3-70b"), 1, 4096)
    assert 68 * per70 <= free_70b - Engine.AUTO_RESERVE_BYTES < 132 * per70
