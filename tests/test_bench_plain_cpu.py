"""bench.py's plain run and ``--dump-outputs``: without ``--full`` the run times its QA steps and
prints the JSON line, nothing else (no latency reps, ingest or phase breakdowns, whatever their
options say); ``--dump-outputs DIR`` writes what the last timed step returned as float32 / float64
.npy files, identical from run to run for the same arguments. Rehearsed on one CPU rank with tiny
configs: the schema and the determinism are pinned here; the numbers come from the GPU."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, STEPS, MAX_NEW, TOP_K = 3, 2, 4, 5


def _run(dump):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["OMP_NUM_THREADS"] = "2"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--cpu-rehearsal",
           "--enc", "tiny-enc", "--llm", "tiny-dec", "--batch", str(B), "--steps", str(STEPS), "--warmup", "1",
           "--index-rows", "2000", "--max-new", str(MAX_NEW), "--top-k", str(TOP_K),
           # --full's options: a plain run must not act on them
           "--latency-reps", "2", "--ingest-docs", "2", "--breakdown", "1",
           "--dump-outputs", str(dump)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_times_only_its_steps_and_dumps_repeatable_outputs(tmp_path):
    out = _run(tmp_path / "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["steps"] == STEPS and out["warmup"] == 1 and out["ms_per_step"] > 0
    # value and ms_per_step describe the same timed steps
    assert abs(out["value"] - B / (out["ms_per_step"] / 1000)) <= 0.01 * out["value"]
    # exactly warmup + steps QA batches were searched, and nothing else ran
    sp = out["search_plane"]
    assert sp["searches"] == STEPS + 1 and sp["rows"] == B * (STEPS + 1), sp
    assert out["latency_reps"] == 0 and out["p50_cache_miss_ms"] is None
    assert out["ingest_docs_per_min"] is None and out["ingest_single_doc_reps"] == 0
    assert out["qa_step_phase_ms"] is None and out["latency_phase_ms"] is None and out["ingest_phase_ms"] is None

    _run(tmp_path / "b")
    shapes = {"query_embeddings": (B, None), "search_scores": (B, TOP_K), "search_ids": (B, TOP_K),
              "answer_codepoints": (B, 32 * MAX_NEW), "answer_chars": (B,), "confidence": (B,)}
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in shapes)
    total = 0
    for name, shape in shapes.items():
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        assert a.ndim == len(shape) and all(s is None or s == n for s, n in zip(shape, a.shape)), (name, a.shape)
        assert np.array_equal(a, b), name
        total += a.nbytes
    assert total <= 64 << 20
    ids, conf = np.load(tmp_path / "a" / "search_ids.npy"), np.load(tmp_path / "a" / "confidence.npy")
    assert ((ids >= 0) & (ids < 2000)).all() and np.isfinite(conf).all()
    chars, cp = np.load(tmp_path / "a" / "answer_chars.npy"), np.load(tmp_path / "a" / "answer_codepoints.npy")
    assert ((cp >= 0).sum(axis=1) == np.minimum(chars, cp.shape[1])).all()
