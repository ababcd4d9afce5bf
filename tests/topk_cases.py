"""Candidate sets for the top-k merge (kernel on the GPU, ops/reference.py on the CPU) and their
oracle: a plain Python sort of (-score, id) over the entries with id >= 0."""
import numpy as np
import torch

MERGE_P = [1, 2, 7, 33]   # 33 x 32 = 1056 candidates: more than the kernel's 256-thread stride
MERGE_Q = [1, 5]
MERGE_K = [1, 8, 32]
EMPTY_QUERY = 3           # with Q = 5: every candidate of this query is empty


def merge_case(P, Q, K):
    """cand_s fp32 [P, Q, K], cand_i int32 [P, Q, K] holding, per query: unique ids up to 1e8, scores
    from a pool with exact ties and one-ulp neighbours around 0.5, ids of -1 under finite scores,
    -inf scores under real ids and under -1, and (two or more candidates) a planted pair whose
    better score sits one ulp above the other's under an id 1e8 larger."""
    rng = np.random.default_rng(P * 1000 + Q * 100 + K)
    n = P * K
    half = np.float32(0.5)
    up, down = np.nextafter(half, np.float32(1)), np.nextafter(half, np.float32(0))
    s = np.empty((Q, n), dtype=np.float32)
    i = np.empty((Q, n), dtype=np.int64)
    for q in range(Q):
        pick = rng.integers(0, 6, n)
        pool = np.stack([np.full(n, half), np.full(n, up), np.full(n, down), np.full(n, np.float32(0.25)),
                         rng.uniform(-1, 0.45, n).astype(np.float32), rng.uniform(-1, 0.45, n).astype(np.float32)])
        s[q] = pool[pick, np.arange(n)]
        ids = np.sort(rng.integers(0, 10 ** 8 - n, n)) + np.arange(n)   # unique, up to 1e8
        i[q] = rng.permutation(ids)
        s[q, rng.random(n) < 0.1] = -np.inf                              # -inf under a real id ...
        i[q, rng.random(n) < 0.15] = -1                                  # ... and empties under any score
        if n >= 2:  # the pair a mixed score/id key gets wrong: first and last candidate (different parts)
            s[q, 0], i[q, 0] = half, 3
            s[q, n - 1], i[q, n - 1] = up, 99_999_937
        if Q > 1 and q == EMPTY_QUERY:
            i[q] = -1
    cs = torch.from_numpy(s.reshape(Q, P, K).transpose(1, 0, 2).copy())
    ci = torch.from_numpy(i.astype(np.int32).reshape(Q, P, K).transpose(1, 0, 2).copy())
    return cs, ci


def merge_oracle(cand_s, cand_i, K):
    """(scores fp32 [Q, K], ids int32 [Q, K]): per query the K first of sorted((-score, id)) over the
    entries with id >= 0, padded with (-inf, -1)."""
    P, Q, _ = cand_s.shape
    s, i = cand_s.cpu().numpy(), cand_i.cpu().numpy()
    os = np.full((Q, K), -np.inf, dtype=np.float32)
    oi = np.full((Q, K), -1, dtype=np.int32)
    for q in range(Q):
        ent = sorted((-float(a), int(b)) for a, b in zip(s[:, q].ravel(), i[:, q].ravel()) if b >= 0)[:K]
        for r, (a, b) in enumerate(ent):
            os[q, r], oi[q, r] = -a, b
    return torch.from_numpy(os), torch.from_numpy(oi)


def assert_merge(got_s, got_i, cand_s, cand_i, K):
    """Scores bit-exact (they are copies), ids exact."""
    os, oi = merge_oracle(cand_s, cand_i, K)
    gs, gi = got_s.cpu(), got_i.cpu()
    assert gs.dtype == torch.float32 and gi.dtype == torch.int32
    assert torch.equal(gi, oi), (gi, oi)
    assert torch.equal(gs.view(torch.int32), os.view(torch.int32)), (gs, os)
