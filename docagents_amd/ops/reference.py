"""Plain-PyTorch fp32 reference implementations of every kernel in ``kernels.py``.

Used as the numerics oracle in tests (HIP kernel vs fp32 PyTorch of the same op) and as the
CPU execution path of the models (the container running CPU tests has no GPU). They are NOT a
GPU fallback: on a GPU device the models always call the HIP kernels.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

EPI_NONE, EPI_BIAS, EPI_GELU, EPI_SWIGLU, EPI_RESID = 0, 1, 2, 3, 4
EPI_ROPE = 6  # gemm8p only: QKV + RoPE + KV-cache write

# No routing rule of its own: these ARE the planner's objects (pure Python), so a CPU decoder takes
# the route the GPU one does. The DECODE_DK switch is read where it lives, gemm_plan.DECODE_DK.
from .gemm_plan import (DK_MAX_M, DK_SPLITK_ABOVE, dk_fusable, dk_parts, dk_w8_fusable,  # noqa: E402,F401
                        gemv_fusable, gemv_w4_fusable, gemv_w8_fusable, keeps_w4_copy, keeps_w8_copy,
                        prefill_w8_fusable, tile_w8_fusable, weight_op)


def gemm_route(M, N, K, epi=EPI_NONE):
    """kernels.gemm_route: gemm() keywords that give a subset of M rows the full launch's routing
    (none needed here: the oracle has one routine), None for M <= 128 as there."""
    return None if M <= 128 else {}


def gemm(a, w, bias=None, epi=EPI_NONE, resid=None, out=None, rms=None, **_):
    if rms is not None:  # same numerics as rmsnorm() followed by gemm() (bf16 normalised row)
        g = rms[0] if rms[0] is not None else torch.ones(a.shape[1], dtype=a.dtype, device=a.device)
        a = rmsnorm(a, g, rms[1])
    return _epilogue(a.float() @ w.float().t(), w.shape[0], bias, epi, resid, out)


def _epilogue(y, N, bias, epi, resid, out):
    if bias is not None:
        y = y + bias.float()
    if epi == EPI_GELU:
        y = F.gelu(y)
    elif epi == EPI_SWIGLU:
        yy = y.view(y.shape[0], N // 32, 2, 16)
        g, u = yy[:, :, 0, :], yy[:, :, 1, :]
        y = (F.silu(g) * u).reshape(y.shape[0], N // 2)
    elif epi == EPI_RESID:
        y = y + resid.float()
    y = y.to(torch.bfloat16)
    if out is not None:
        out.copy_(y)
        return out
    return y


def gemm_f16(a, w, bias=None, epi=EPI_NONE, resid=None, out=None):
    """fp16 oracle of kernels.gemm_f16: fp32 product + epilogue, one fp16 rounding."""
    y = a.float() @ w.float().t()
    if bias is not None:
        y = y + bias.float()
    if epi == EPI_GELU:
        y = F.gelu(y)
    elif epi == EPI_RESID:
        y = y + resid.float()
    y = y.to(torch.float16)
    if out is not None:
        out.copy_(y)
        return out
    return y


def interleave_gate_up(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    """[F, K] gate + [F, K] up -> [2F, K] rows interleaved in 16-row groups (EPI_SWIGLU layout)."""
    Fd, K = gate.shape
    assert Fd % 16 == 0
    g = gate.view(Fd // 16, 16, K)
    u = up.view(Fd // 16, 16, K)
    return torch.stack([g, u], dim=1).reshape(2 * Fd, K).contiguous()


def rmsnorm(x, w, eps, resid=None, out=None, route_m=0):
    xf = x.float()
    if resid is not None:
        xf = xf + resid.float()
        resid.copy_(xf.to(resid.dtype))
    y = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * w.float()
    y = y.to(x.dtype)
    if out is not None:
        out.copy_(y)
        return out
    return y


def layernorm(x, g, b, eps, resid=None, out=None, fp8_out=False):
    xf = x.float()
    if resid is not None:
        xf = xf + resid.float()
    yf = F.layer_norm(xf, (xf.shape[-1],), g.float(), None if b is None else b.float(), eps)
    y = yf.to(x.dtype)
    if out is not None:
        out.copy_(y)
        y = out
    if fp8_out:
        yq, ys = quant_fp8(yf)
        return y, yq, ys
    return y


def bert_embed_ln(ids, positions, types, word, pos, type_, g, b, eps, out=None, fp8_out=False):
    t = type_[types.long()] if types is not None else type_[0]
    x = word[ids.long()].float() + pos[positions.long()].float() + t.float()
    return layernorm(x.to(word.dtype), g, b, eps, out=out, fp8_out=fp8_out)


def embed(ids, table, out=None):
    y = table[ids.long()]
    if out is not None:
        out.copy_(y)
        return out
    return y


def pool_l2norm(h, cu_seqlens, mode=0, out32=None, out16=None):
    cu = cu_seqlens.tolist()
    rows = []
    for i in range(len(cu) - 1):
        s0, s1 = cu[i], cu[i + 1]
        if mode == 0 or s1 <= s0:
            rows.append(h[s0].float())
        else:
            rows.append(h[s0:s1].float().mean(0))
    v = torch.stack(rows) if rows else torch.zeros((0, h.shape[1]))
    n = v.norm(dim=-1, keepdim=True)
    v = torch.where(n > 0, v / n.clamp_min(1e-30), v)
    if out16 is not None:
        out16.copy_(v.to(out16.dtype))
    if out32 is not None:
        out32.copy_(v)
        return out32
    return v if out16 is None else out16


def rope_table(max_pos: int, D: int, theta: float, device=None) -> torch.Tensor:
    inv = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.float64) / D))
    t = torch.arange(max_pos, dtype=torch.float64)
    ang = torch.outer(t, inv)
    return torch.stack([ang.cos(), ang.sin()], dim=-1).float().contiguous().to(device)


def _rope_rows(x, cs):  # x [T, nh, D], cs [T, D/2, 2]; pairs (2i, 2i+1) rotated by theta_i * pos
    x1, x2 = x[..., 0::2].float(), x[..., 1::2].float()
    c, s = cs[:, None, :, 0], cs[:, None, :, 1]
    return torch.stack([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).flatten(-2)


def gemm_rope(a, w, pos, cos_sin, H, Hkv, D, slot, k_cache, v_cache, out=None, kv_out=True):
    """QKV projection with RoPE on q / k and the k / v cache write fused (gemm + rope_cache)."""
    qkv = gemm(a, w, out=out)
    return rope_cache(qkv, pos, cos_sin, H, Hkv, D, slot=slot, k_cache=k_cache, v_cache=v_cache)


def rope_cache(qkv, pos, cos_sin, H, Hkv, D, slot=None, k_cache=None, v_cache=None, rotate_q=True):
    T = qkv.shape[0]
    x = qkv.view(T, H + 2 * Hkv, D)
    cs = cos_sin[pos.long()]
    if rotate_q:
        x[:, :H] = _rope_rows(x[:, :H], cs).to(qkv.dtype)
    x[:, H:H + Hkv] = _rope_rows(x[:, H:H + Hkv], cs).to(qkv.dtype)
    if k_cache is not None:
        sl, ps = slot.long(), pos.long()
        k_cache[sl, :, ps] = x[:, H:H + Hkv]
        v_cache[sl, :, ps] = x[:, H + Hkv:]
    return qkv


def flash_kv_cache_ok(D: int, causal: bool) -> bool:
    return causal


def flash_attn_varlen(q, k, v, cu_seqlens, max_seqlen, H, Hkv, D, causal, scale=None, out=None, prefix=None,
                      kv_cache=None, tail_only=False):
    """prefix = (k_pre [Hkv, >=P, D], v_pre, P): every sequence's keys are the P shared prefix keys
    followed by its own; query i sits at key position P + i (bottom-right causal).
    kv_cache = (k_cache, v_cache, slot, pos): own keys of the sequence starting at token t read from
    k_cache[slot[t], :, pos[t] + j] (k / v ignored).
    tail_only: only the 128-row query block holding each sequence's last token is defined (computed
    as in a full call, so the same bits); the other rows, which the kernel leaves unwritten, are NaN
    here so that a consumer of one shows up."""
    if kv_cache is not None:
        kc, vc, ks, kpos = kv_cache
        T = q.shape[0]
        cu = cu_seqlens.tolist()
        k = torch.empty((T, Hkv * D), dtype=q.dtype, device=q.device)
        v = torch.empty((T, Hkv * D), dtype=q.dtype, device=q.device)
        for b in range(len(cu) - 1):
            s0, s1 = cu[b], cu[b + 1]
            if s1 > s0:
                sl, p0 = int(ks[s0]), int(kpos[s0])
                k[s0:s1] = kc[sl, :, p0:p0 + s1 - s0].transpose(0, 1).reshape(s1 - s0, Hkv * D)
                v[s0:s1] = vc[sl, :, p0:p0 + s1 - s0].transpose(0, 1).reshape(s1 - s0, Hkv * D)
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    T = q.shape[0]
    res = torch.empty((T, H * D), dtype=q.dtype, device=q.device)
    cu = cu_seqlens.tolist()
    G = H // Hkv
    P = 0 if prefix is None else int(prefix[2])
    if P:
        kp = prefix[0][:, :P].float().repeat_interleave(G, 0)   # [H, P, D]
        vp = prefix[1][:, :P].float().repeat_interleave(G, 0)
    for b in range(len(cu) - 1):
        s0, s1 = cu[b], cu[b + 1]
        L = s1 - s0
        if L == 0:
            continue
        qq = q[s0:s1, :H * D].float().view(L, H, D).transpose(0, 1)
        kk = k[s0:s1, :Hkv * D].float().view(L, Hkv, D).transpose(0, 1).repeat_interleave(G, 0)
        vv = v[s0:s1, :Hkv * D].float().view(L, Hkv, D).transpose(0, 1).repeat_interleave(G, 0)
        if P:
            kk, vv = torch.cat([kp, kk], 1), torch.cat([vp, vv], 1)
        s = (qq @ kk.transpose(1, 2)) * scale
        if causal:
            m = torch.ones(L, P + L, dtype=torch.bool, device=q.device).triu(P + 1)
            s = s.masked_fill(m, float("-inf"))
        p = s.softmax(-1)
        res[s0:s1] = (p @ vv).transpose(0, 1).reshape(L, H * D).to(q.dtype)
        if tail_only:
            res[s0:s0 + (L - 1) // 128 * 128] = float("nan")
    if out is not None:
        out.copy_(res)
        return out
    return res


def decode_attn(q, k_cache, v_cache, lens, slot, H, Hkv, D, max_len=None, chunk=256, scale=None, out=None, pre=None,
                rope=None):
    """pre: optional int32 [B, 2] = (P, prefix slot): keys [0, P) of row b come from the prefix slot.
    rope = (cos_sin, pos): q is the raw qkv row; RoPE + the new token's cache write happen here
    (rope_cache on a copy of the rows, then attention)."""
    if rope is not None:
        q = rope_cache(q.clone(), rope[1], rope[0], H, Hkv, D, slot=slot, k_cache=k_cache, v_cache=v_cache)
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    B = q.shape[0]
    G = H // Hkv
    res = torch.empty((B, H * D), dtype=q.dtype, device=q.device)
    pre_h = None if pre is None else pre.tolist()
    for b in range(B):
        L, s = int(lens[b]), int(slot[b])
        qq = q[b, :H * D].float().view(H, 1, D)
        kk = k_cache[s, :, :L].float()
        vv = v_cache[s, :, :L].float()
        if pre_h is not None and pre_h[b][0] > 0:
            P, ps = pre_h[b]
            kk = torch.cat([k_cache[ps, :, :P].float(), kk[:, P:]], 1)
            vv = torch.cat([v_cache[ps, :, :P].float(), vv[:, P:]], 1)
        kk, vv = kk.repeat_interleave(G, 0), vv.repeat_interleave(G, 0)
        p = ((qq @ kk.transpose(1, 2)) * scale).softmax(-1)
        res[b] = (p @ vv).reshape(H * D).to(q.dtype)
    if out is not None:
        out.copy_(res)
        return out
    return res


def log_softmax_rows(logits):
    return torch.log_softmax(logits.float(), dim=-1)


_M32 = 0xFFFFFFFF


def _hash_u32(x: np.ndarray) -> np.ndarray:
    """common.h hash_u32 on uint32 arrays (numpy uint32 arithmetic wraps mod 2^32, like the kernel)."""
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def gumbel_u01(seed: int, rkey, v) -> np.ndarray:
    """The sampler kernel's counter-based uniform (common.h u01(seed, rkey, v)), bit-exact; rkey and
    v broadcast (uint32-valued integer arrays)."""
    with np.errstate(over="ignore"):
        rk = np.asarray(rkey, dtype=np.uint32)
        vv = np.asarray(v, dtype=np.uint32)
        inner = _hash_u32(vv + np.uint32(0x632be5ab))
        h = _hash_u32(np.uint32(seed & _M32) ^ _hash_u32(rk + np.uint32(0x9e3779b9) * inner))
    return ((h >> np.uint32(8)).astype(np.float64) + 0.5) * (1.0 / 16777216.0)


def _gumbel_scores(x, temperature, seed, rkeys, v0=0):
    """x fp32 [B, V] -> Gumbel-max scores x / T - log(-log u(seed, rkey_b, v0 + v)) (T <= 0: x)."""
    if temperature <= 0:
        return x.double()
    B, V = x.shape
    u = gumbel_u01(seed, rkeys.reshape(B, 1), np.arange(v0, v0 + V, dtype=np.int64).reshape(1, V))
    return x.double().cpu() / temperature - torch.from_numpy(np.log(-np.log(u)))


def _rkeys(B, step, ctr) -> np.ndarray:
    rs = (ctr.cpu().numpy()[:B].astype(np.int64) if ctr is not None else np.full(B, step, dtype=np.int64))
    with np.errstate(over="ignore"):
        return rs.astype(np.uint32) * np.uint32(131071) + np.arange(B, dtype=np.uint32)


def _bookkeep(B, tok, chosen, device, out_tok=None, out_lp=None, conf=None, active=None, pos=None, lens=None,
              hist=None, start=None, eos=()):
    on = active.bool().clone() if active is not None else torch.ones(B, dtype=torch.bool, device=device)
    if out_tok is None:
        out_tok = torch.zeros(B, dtype=torch.int32, device=device)
    out_tok.copy_(torch.where(on, tok, out_tok))
    if out_lp is not None:
        out_lp.copy_(torch.where(on, chosen, out_lp))
    if conf is not None:
        conf[:, 0] += torch.where(on, chosen.exp(), torch.zeros_like(chosen))
        conf[:, 1] += on.float()
    stop = torch.zeros(B, dtype=torch.bool, device=device)
    for e in list(eos)[:4]:
        stop |= tok == e
    if hist is not None:
        gi = (pos - start).long()
        for b in range(B):
            if on[b] and 0 <= gi[b] < hist.shape[1]:
                hist[b, gi[b]] = tok[b]
        stop |= (gi + 1) >= hist.shape[1]
    if pos is not None:
        pos += on.int()
    if lens is not None:
        lens += on.int()
    if active is not None:
        active.copy_(torch.where(on & stop, torch.zeros_like(active), active))
    return out_tok, chosen


def sample(logits, temperature, seed, step=0, out_tok=None, out_lp=None, conf=None, active=None, ctr=None,
           pos=None, lens=None, hist=None, start=None, eos=()):
    """Reference sampler with the kernel's semantics: Gumbel-max at temperature T with the kernel's
    counter-based hash noise (greedy when T <= 0; ties to the lower index), the chosen token's
    log-probability under the untempered distribution, and the device-side bookkeeping."""
    B = logits.shape[0]
    lp = log_softmax_rows(logits)
    sc = _gumbel_scores(logits.float().cpu(), temperature, seed, _rkeys(B, step, ctr))
    tok = sc.argmax(-1).to(logits.device)  # first maximal index = the kernel's lower-index tie rule
    chosen = lp.gather(1, tok.view(-1, 1)).squeeze(1)
    return _bookkeep(B, tok.int(), chosen, logits.device, out_tok, out_lp, conf, active, pos, lens, hist, start, eos)


def sample_partial(logits, temperature, seed, v0, step=0, ctr=None, out=None):
    """Vocab-parallel sampling, rank side (see ops.kernels.sample_partial): stats fp32 [B, 8]."""
    B, V = logits.shape
    x = logits.float().cpu()
    sc = _gumbel_scores(x, temperature, seed, _rkeys(B, step, ctr), v0)
    bi = sc.argmax(-1)
    mx = x.max(-1).values
    st = torch.zeros((B, 8), dtype=torch.float32)
    st[:, 0] = sc.gather(1, bi.view(-1, 1)).squeeze(1).float()
    st[:, 1] = (bi + v0).to(torch.int32).view(torch.float32)
    st[:, 2] = mx
    st[:, 3] = torch.exp(x - mx[:, None]).sum(-1)
    st[:, 4] = x.gather(1, bi.view(-1, 1)).squeeze(1)
    st = st.to(logits.device)
    if out is not None:
        out.copy_(st)
        return out
    return st


def sample_finalize(gathered, ranks, out_tok=None, out_lp=None, conf=None, active=None, pos=None, lens=None,
                    hist=None, start=None, eos=()):
    """Vocab-parallel sampling, merge side: gathered [B, ranks * 8] -> sample()'s outputs."""
    B = gathered.shape[0]
    g = gathered.float().cpu().view(B, ranks, 8)
    score, idx = g[..., 0], g[..., 1].contiguous().view(torch.int32).long()
    best = score.max(-1).values
    cand = torch.where(score == best[:, None], idx, torch.full_like(idx, 1 << 40))
    r = cand.argmin(-1)  # max score, ties to the lower global index
    tok = idx.gather(1, r.view(-1, 1)).squeeze(1)
    xb = g[..., 4].gather(1, r.view(-1, 1)).squeeze(1).double()
    gmax = g[..., 2].max(-1).values.double()
    lse = gmax + torch.log((g[..., 3].double() * torch.exp(g[..., 2].double() - gmax[:, None])).sum(-1))
    chosen = (xb - lse).float().to(gathered.device)
    return _bookkeep(B, tok.int().to(gathered.device), chosen, gathered.device, out_tok, out_lp, conf, active, pos,
                     lens, hist, start, eos)


def topk_dense(X, Qv, K, thr, slots=None, bitmap=None, **_):
    s = Qv.float() @ X.float().t()  # [Q, N]
    valid = s >= thr
    if slots is not None:
        valid &= (slots[:X.shape[0]] >= 0).view(1, -1)
    if bitmap is not None:
        sl = slots[:X.shape[0]].long().clamp_min(0)
        words = bitmap[:, (sl >> 5)]  # [Q, N]
        bits = (words >> (sl & 31).view(1, -1)) & 1
        valid &= bits.bool()
    s = s.masked_fill(~valid, float("-inf"))
    return _topk_with_ties(s, K)


def _topk_with_ties(s, K):
    Q, N = s.shape
    if N == 0:
        return (torch.full((Q, K), float("-inf")), torch.full((Q, K), -1, dtype=torch.int32))
    # sort desc by score, asc by index
    idx = torch.arange(N, device=s.device).expand(Q, N)
    order = torch.argsort(idx, dim=1, stable=True)
    vals, perm = torch.sort(s, dim=1, descending=True, stable=True)
    ids = torch.gather(idx, 1, perm)
    kk = min(K, N)
    vs, ii = vals[:, :kk], ids[:, :kk].int()
    ii = torch.where(torch.isinf(vs), torch.full_like(ii, -1), ii)
    if kk < K:
        vs = torch.cat([vs, torch.full((Q, K - kk), float("-inf"), device=s.device)], 1)
        ii = torch.cat([ii, torch.full((Q, K - kk), -1, dtype=torch.int32, device=s.device)], 1)
    del order
    return vs, ii


def topk_ranges(X, Qv, ranges, range_off, K, thr, max_rows=None, slots=None, bitmap=None, **_):
    Q = Qv.shape[0]
    N = X.shape[0]
    s = Qv.float() @ X.float().t()
    allowed = torch.zeros((Q, N), dtype=torch.bool, device=X.device)
    ro = range_off.tolist()
    rg = ranges.tolist()
    for q in range(Q):
        for r in range(ro[q], ro[q + 1]):
            a, b = rg[r]
            allowed[q, a:b] = True
    valid = allowed & (s >= thr)
    if slots is not None:
        valid &= (slots[:N] >= 0).view(1, -1)
    if bitmap is not None:
        sl = slots[:N].long().clamp_min(0)
        bits = (bitmap[:, (sl >> 5)] >> (sl & 31).view(1, -1)) & 1
        valid &= bits.bool()
    s = s.masked_fill(~valid, float("-inf"))
    return _topk_with_ties(s, K)


def topk_merge(cand_s, cand_i, K):
    P, Q, _ = cand_s.shape
    s = cand_s.permute(1, 0, 2).reshape(Q, -1)
    i = cand_i.permute(1, 0, 2).reshape(Q, -1)
    empty = i < 0
    s = torch.where(empty, torch.full_like(s, float("-inf")), s)
    i = torch.where(empty, torch.full_like(i, -1), i)
    # lexicographic, as better() of csrc/vecsearch_topk.h: score desc, then id asc, empties (id < 0)
    # last. Three stable sorts, least significant key first (a single mixed key such as
    # score * 1e12 - id lets a large id difference outweigh a one-ulp score difference).
    order = torch.argsort(i, dim=1, stable=True)
    order = torch.gather(order, 1, torch.argsort(torch.gather(s, 1, order), dim=1, descending=True, stable=True))
    order = torch.gather(order, 1, torch.argsort(torch.gather(empty, 1, order).to(torch.uint8), dim=1, stable=True))
    return torch.gather(s, 1, order)[:, :K], torch.gather(i, 1, order)[:, :K]


def kmeans_accum(X, assign, sums, counts):
    a = assign.long()
    m = a >= 0
    sums.index_add_(0, a[m], X[m].float())
    counts.index_add_(0, a[m], torch.ones(int(m.sum()), device=X.device))


# ----------------------------------------------------------------------------------- fp8 path
def quant_fp8(x, out=None, scale=None):
    xf = x.float()
    sc = xf.abs().amax(dim=1) / 448.0
    sc = torch.where(sc > 0, sc, torch.ones_like(sc))
    q = (xf / sc[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn)
    if out is not None:
        out.copy_(q)
        q = out
    if scale is not None:
        scale[:sc.numel()].copy_(sc)
        sc = scale
    return q, sc


def gemm_fp8(aq, sa, wq, sw, bias=None, epi=EPI_NONE, resid=None, out=None):
    y = (aq.float() * sa[:aq.shape[0], None].float()) @ (wq.float() * sw[:, None].float()).t()
    return _epilogue(y, wq.shape[0], bias, epi, resid, out)


def rmsnorm_q8(x, g, eps, out=None, scale=None, route_m=0):
    """fp32 oracle of kernels.rmsnorm_q8: the normalised row rounded to bf16 (rmsnorm), then
    quant_fp8's per-row rule -> (codes [M, D] float8_e4m3fn, scale [M] fp32)."""
    return quant_fp8(rmsnorm(x, g, eps), out=out, scale=scale)


def quant_weight_fp8(w):
    """Per-output-channel e4m3 weight quantisation (host-side torch; done once at load)."""
    wf = w.float()
    sw = (wf.abs().amax(dim=1) / 448.0).clamp_min(1e-30)
    return (wf / sw[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn).contiguous(), sw.contiguous()


def quant_weight_fp8_pow2(w):
    """Per-output-row e4m3 quantisation with a power-of-two row scale (host-side torch; done once at
    load): s = the smallest 2^e with amax_row / 2^e <= 448 (all-zero rows: 1). An e4m3 value times a
    power of two is exact in bf16, so ``q.float() * s[:, None]`` IS a bf16 matrix: the bf16 kernels
    and the fp8 kernels compute the same model. Returns (q [N, K] float8_e4m3fn, s [N] fp32)."""
    wf = w.float()
    amax = wf.abs().amax(dim=1)
    s = torch.exp2(torch.ceil(torch.log2(amax.clamp_min(2.0 ** -100) / 448.0)))
    s = torch.where(amax / s > 448.0, s * 2, s)        # log2 rounding at an exact power-of-two ratio
    s = torch.where(amax / (s / 2) <= 448.0, s / 2, s)
    s = torch.where(amax > 0, s, torch.ones_like(s))
    return (wf / s[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn).contiguous(), s.contiguous()


# ----------------------------------------------------------------------------------- MXFP4 weights
# OCP microscaling fp4: e2m1 codes (sign in bit 3, magnitude index into E2M1_GRID in bits 2:0), two
# per byte (element 2j in bits 3:0 of byte j, element 2j+1 in bits 7:4), and one e8m0 scale byte
# (e + 127) per 32 consecutive elements of a row.
E2M1_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
MX_BLOCK = 32


def quant_weight_mxfp4(w):
    """MXFP4 weight quantisation (host-side torch; done once at load) -> (codes uint8 [N, K/2],
    scales uint8 [N, K/32]); K % 32 == 0. Per block of 32 consecutive k of a row: e = the smallest
    integer with amax / 2^e <= 6 (no clipping: the rule of quant_weight_fp8_pow2, not the OCP floor
    rule), clamped to [-126, 127], 0 for an all-zero block; the byte is e + 127, so bytes 0 and 255
    (the e8m0 NaN) never occur. w / 2^e is rounded to the nearest of E2M1_GRID, ties to the even
    mantissa (0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4); what rounds to
    zero is stored as code 0, never -0. An e2m1 value times a power of two is exact in bf16, so
    dequant_mxfp4 of the result IS a bf16 matrix (magnitudes above 3.5 * 2^126, which no weight has,
    would round up to 2^128, past the bf16 range)."""
    N, K = w.shape
    if K % MX_BLOCK:
        raise ValueError(f"quant_weight_mxfp4 needs K % {MX_BLOCK} == 0, got K={K}")
    wf = w.float().reshape(N, K // MX_BLOCK, MX_BLOCK)
    amax = wf.abs().amax(dim=-1)
    # amax = m * 2^x, m in [0.5, 1); 6 = 0.75 * 2^3: amax / 2^e <= 6 <=> e >= x - 3 (m <= 0.75), x - 2 (else)
    m, x = torch.frexp(amax)
    e = (x - 3 + (m > 0.75).to(x.dtype)).clamp(-126, 127)
    e = torch.where(amax > 0, e, torch.zeros_like(e))
    v = torch.ldexp(wf, -e[..., None])
    a = v.abs()
    # the index on the grid: one step per midpoint passed; a tie stays below an odd index and goes up to an even one
    idx = ((a > 0.25).to(torch.uint8) + (a >= 0.75) + (a > 1.25) + (a >= 1.75) + (a > 2.5) + (a >= 3.5) + (a > 5.0))
    code = (idx | (((v < 0) & (idx > 0)).to(torch.uint8) << 3)).reshape(N, K)
    packed = (code[:, 0::2] | (code[:, 1::2] << 4)).contiguous()
    return packed, (e + 127).to(torch.uint8).contiguous()


def dequant_mxfp4(codes, scales):
    """bf16 [N, K] of MXFP4 codes [N, K/2] and scale bytes [N, K/32]: exact (see quant_weight_mxfp4)."""
    N, K = codes.shape[0], codes.shape[1] * 2
    c = torch.stack([codes & 0xF, codes >> 4], dim=-1).reshape(N, K).long()
    grid = torch.tensor(E2M1_GRID, dtype=torch.float32, device=codes.device)
    val = torch.where((c & 8) != 0, -grid[c & 7], grid[c & 7])
    e = (scales.to(torch.int32) - 127).repeat_interleave(MX_BLOCK, dim=1)
    return torch.ldexp(val, e).to(torch.bfloat16)


def gemm_w4(a, wq, se, bias=None, epi=EPI_NONE, resid=None, out=None, rms=None):
    """gemv_w4.hip: gemm() (with its fused RMSNorm on the bf16-normalised row) on the dequantised matrix."""
    return gemm(a, dequant_mxfp4(wq, se), bias=bias, epi=epi, resid=resid, out=out, rms=rms)


# ----------------------------------------------------------------------------------- fp8 vector index
# codes [N, d] (uint8 / float8_e4m3fn) + scale fp32 [N]: every row is quant_weight_fp8_pow2 of the
# bf16 row, so codes * scale is exact in bf16 and the fp8 searches ARE the bf16 searches of that matrix.
DENSE8_DIMS = (128, 384, 768, 1024)


def index_dequant(codes, scale):
    """bf16 [N, d]: codes * scale (exact)."""
    c = codes.view(torch.float8_e4m3fn) if codes.dtype == torch.uint8 else codes
    return (c.float() * scale[:c.shape[0], None].float()).to(torch.bfloat16)


def index_quant_rows(X, codes, scale, row0=0, dest=None):
    """Rows [row0, row0 + n) of codes / scale <- quant_weight_fp8_pow2(X); with ``dest`` (int64 [n],
    distinct rows) row r of X goes to row dest[r] instead."""
    n = X.shape[0]
    q, s = quant_weight_fp8_pow2(X.to(torch.bfloat16))
    if dest is not None:
        if row0 != 0:
            raise ValueError("dest and row0 exclude each other")
        if n and (int(dest.min()) < 0 or int(dest.max()) >= codes.shape[0]):
            raise ValueError(f"dest names rows outside [0, {codes.shape[0]})")
        codes.view(torch.uint8)[dest] = q.view(torch.uint8)
        scale[dest] = s
        return codes, scale
    codes.view(torch.uint8)[row0:row0 + n] = q.view(torch.uint8)
    scale[row0:row0 + n] = s
    return codes, scale


def index_dequant_rows(codes, scale, out, row0=0, sel=None):
    """out [n, d] bf16 <- index_dequant of rows row0 .. row0 + n, or of the rows ``sel`` (int64 [n])."""
    n = out.shape[0]
    if sel is not None:
        if row0 != 0:
            raise ValueError("sel and row0 exclude each other")
        if n and (int(sel.min()) < 0 or int(sel.max()) >= codes.shape[0]):
            raise ValueError(f"sel names rows outside [0, {codes.shape[0]})")
        out.copy_(index_dequant(codes.index_select(0, sel), scale.index_select(0, sel)))
    else:
        if row0 < 0 or row0 + n > codes.shape[0]:
            raise ValueError("rows [row0, row0 + n) outside codes")
        out.copy_(index_dequant(codes[row0:row0 + n], scale[row0:row0 + n]))
    return out


def kmeans_accum8(codes, scale, assign, sums, counts):
    kmeans_accum(index_dequant(codes, scale), assign, sums, counts)


def topk_dense8(codes, scale, Qv, K, thr, slots=None, bitmap=None, **_):
    return topk_dense(index_dequant(codes, scale), Qv, K, thr, slots=slots, bitmap=bitmap)


def topk_ranges8(codes, scale, Qv, ranges, range_off, K, thr, max_rows=None, slots=None, bitmap=None, **_):
    return topk_ranges(index_dequant(codes, scale), Qv, ranges, range_off, K, thr, max_rows=max_rows, slots=slots,
                       bitmap=bitmap)


# ----------------------------------------------------------------------------------- fp8 KV cache
# codes [slots, Hkv, max_seq, D] float8_e4m3fn + scales [slots, Hkv, max_seq] fp32: every cached row
# is quant_weight_fp8_pow2 of the bf16 row (power-of-two scale: code * scale is exact in bf16).
def kv8_dequant_all(codes, scale):
    """The whole cache tensor (any leading dims) dequantised to bf16 (exact)."""
    return (codes.float() * scale[..., None].float()).to(torch.bfloat16)


def rope_cache_kv8(qkv, pos, cos_sin, H, Hkv, D, slot, k_codes, v_codes, k_scale, v_scale, rotate_q=True):
    """rope_cache on qkv (in place, the same roundings), then the rotated k row and the v row of every
    (token, kv head) quantised into the fp8 cache at [slot[t], :, pos[t]]."""
    T = qkv.shape[0]
    rope_cache(qkv, pos[:T], cos_sin, H, Hkv, D, rotate_q=rotate_q)
    x = qkv.view(T, H + 2 * Hkv, D)
    sl, ps = slot[:T].long(), pos[:T].long()
    for rows, codes, scale in ((x[:, H:H + Hkv], k_codes, k_scale), (x[:, H + Hkv:], v_codes, v_scale)):
        q, s = quant_weight_fp8_pow2(rows.reshape(T * Hkv, D))
        codes.view(torch.uint8)[sl, :, ps] = q.view(torch.uint8).view(T, Hkv, D)  # index_put on bytes
        scale[sl, :, ps] = s.view(T, Hkv)
    return qkv


def decode_attn_kv8(q, k_codes, v_codes, k_scale, v_scale, lens, slot, H, Hkv, D, max_len=None, chunk=0, scale=None,
                    out=None, pre=None):
    """decode_attn over the dequantised cache (dequantisation is exact in bf16, so this IS decode_attn
    on a bf16 cache that holds those values). Only the slots the call reads are dequantised."""
    used = set(int(s) for s in slot.tolist())
    if pre is not None:
        used |= set(int(p[1]) for p in pre.tolist() if p[0] > 0)
    idx = torch.tensor(sorted(used), dtype=torch.long, device=k_codes.device)
    remap = {s: i for i, s in enumerate(idx.tolist())}
    kc = kv8_dequant_all(k_codes.view(torch.uint8)[idx].view(k_codes.dtype), k_scale[idx])
    vc = kv8_dequant_all(v_codes.view(torch.uint8)[idx].view(v_codes.dtype), v_scale[idx])
    slot2 = torch.tensor([remap[int(s)] for s in slot.tolist()], dtype=torch.int32, device=slot.device)
    pre2 = None
    if pre is not None:
        pre2 = torch.tensor([[p[0], remap[int(p[1])] if p[0] > 0 else 0] for p in pre.tolist()], dtype=torch.int32,
                            device=pre.device).view(-1, 2)
    return decode_attn(q, kc, vc, lens, slot2, H, Hkv, D, max_len=max_len, scale=scale, out=out, pre=pre2)


def kv8_dequant(codes, scale, slot, P):
    """bf16 [Hkv, P, D]: the first P keys of one slot, dequantised (the flash prefill's shared prefix)."""
    slot, P = int(slot), int(P)
    return kv8_dequant_all(codes[slot, :, :P], scale[slot, :, :P]).contiguous()


def gemm_w8(a, wq, sw, bias=None, epi=EPI_NONE, resid=None, out=None, rms=None):
    if rms is not None:  # as gemm(): the bf16 normalised row
        g = rms[0] if rms[0] is not None else torch.ones(a.shape[1], dtype=a.dtype, device=a.device)
        a = rmsnorm(a, g, rms[1])
    return _epilogue((a.float() @ wq.float().t()) * sw[None, :].float(), wq.shape[0], bias, epi, resid, out)


def gemm_dk(a, w, epi=EPI_NONE, bias=None, resid=None, out=None, norm_in=None, ssq_out=None):
    """gemm_dk.hip: optional deferred row RMSNorm of ``a`` from partial sums of squares, then the
    product + epilogue; EPI_RESID may also emit the new rows' per-part sums of squares."""
    M, K = a.shape
    N = w.shape[0]
    x = a.float()
    if norm_in is not None:
        ssq, parts, eps = norm_in
        inv = torch.rsqrt(ssq.view(-1, 64)[:parts, :M].sum(0) / K + eps)
        x = (x * inv[:, None]).to(torch.bfloat16).float()
    y = _epilogue(x @ w.float().t(), N, bias, epi, resid, out)
    if ssq_out is not None:
        parts = dk_parts(N, M)
        bn = -(-N // parts)
        y2 = y.float().pow(2)
        sq = torch.stack([y2[:, i * bn:(i + 1) * bn].sum(-1) for i in range(parts)])  # [parts, M]
        ssq_out.view(-1, 64)[:parts, :M] = sq
    return y


def gemm_dk_w8(a, wq, sw, epi=EPI_NONE, bias=None, resid=None, out=None, norm_in=None, ssq_out=None):
    """gemm_dk_w8.hip: gemm_dk on the dequantised matrix wq * sw, held in fp32. With the decoder's
    power-of-two scales those values are exact in bf16 and this is bit for bit gemm_dk on the bf16
    matrix; an arbitrary fp32 scale is not rounded to bf16 here (the kernel does not round it either:
    rounded weights moved a SwiGLU output with a cancelling up-sum by 0.06, twice the kernel tests' atol)."""
    w = wq.float() * sw[:, None].float()
    return gemm_dk(a, w, epi=epi, bias=bias, resid=resid, out=out, norm_in=norm_in, ssq_out=ssq_out)


def gemm_resid_norm(a, w, resid, gamma, eps, out=None, h_out=None, bias=None):
    y = gemm(a, w, bias=bias, epi=EPI_RESID, resid=resid)
    (resid if out is None else out).copy_(y)
    h = rmsnorm(y, gamma, eps)
    if h_out is not None:
        h_out.copy_(h)
        return h_out
    return h


# The 33..128-row decode products on the e4m3 weight copy (csrc/gemm_tile_w8.hip): each is the bf16
# form's reference op on the dequantised matrix wq * sw (held in fp32, as gemm_dk_w8 holds it).
def _dequant_w8(wq, sw):
    return wq.float() * sw[:, None].float()


def gemm_tile_w8(a, wq, sw, epi=EPI_NONE, bias=None, resid=None, out=None):
    return gemm(a, _dequant_w8(wq, sw), bias=bias, epi=epi, resid=resid, out=out)


def gemm_dk_splitk_w8(a, wq, sw, epi=EPI_NONE, bias=None, resid=None, out=None, norm_in=None, ssq_out=None):
    return gemm_dk(a, _dequant_w8(wq, sw), epi=epi, bias=bias, resid=resid, out=out, norm_in=norm_in, ssq_out=ssq_out)


def gemm_resid_norm_w8(a, wq, sw, resid, gamma, eps, out=None, h_out=None, bias=None):
    return gemm_resid_norm(a, _dequant_w8(wq, sw), resid, gamma, eps, out=out, h_out=h_out, bias=bias)


# fp16 forms of the encoder ops (kernels.*_f16): these references keep the input dtype
layernorm_f16 = layernorm
bert_embed_ln_f16 = bert_embed_ln
pool_l2norm_f16 = pool_l2norm


def flash_attn_f16(q, k, v, cu_seqlens, max_seqlen, H, Hkv, D, causal=False, scale=None, out=None):
    y = flash_attn_varlen(q.float(), k.float(), v.float(), cu_seqlens, max_seqlen, H, Hkv, D, causal, scale=scale)
    y = y.to(torch.float16)
    if out is not None:
        out.copy_(y)
        return out
    return y
