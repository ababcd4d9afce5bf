"""Probe-key inputs for the attention kernels (decode, fp8-cache decode, flash prefill): inputs on
which ONE wrong key moves an output element by >= 1.0, so the suite's usual criterion
(atol = rtol = 0.02 against ops/reference.py) sees it. Pure torch; importable without a GPU.

Uniform mode: every key is zero, so every score is 0 and every visible key weighs exactly 1/n (q is
random: it must not matter). V is zero except probes, V[kv head, key j, col] = A with A a power of
two >= the largest visible key count: an included probe's column reads A/n >= 1, an excluded one 0.
Spike mode: the queries of kv head hk are one unit direction u_hk (16 entries of +-1/4) and one or
two spike keys per row are kappa * sign(u_hk) on u's support, so their score is
beta' = 4 kappa / sqrt(D) (kappa = beta sqrt(D) / 4 rounded to 4 significant bits: exact in bf16,
fp16 and e4m3) and every other score stays 0; A >= n + sum e^beta'.

One launch carries one probe per (kv head, column); key j is probed in layout j // (Hkv D) at
column j % D of kv head (j % (Hkv D) // D + layout) % Hkv. A case yields as many layouts as its
longest row needs and records what it probed; assert_covered() asserts that no key of any row was
left out (decode: the 64 keys past the row's length too, which must read 0). Cache positions that no
correct kernel reads hold A in every column of V: a stray read is loud.

check_reference() asserts the condition that makes the 0.02 tolerance sharp, on the reference's own
output: every included probe >= 1.0, every other element exactly 0."""
import math

import numpy as np
import torch

ATOL = RTOL = 0.02  # the suite's _close(atol=0.02, rtol=0.02)
TILE = 64
DECODE_LENS = [1, 63, 64, 65, 511, 512, 513, 2935, 4000]
# rows ending on a split boundary of the balanced splits (64 (nsplit - 1) keys: the last split empty)
# for the capacity grid of 4096 keys at chunk 1024 / 512 / 256 / 64, and three more odd lengths
DECODE_BOUNDARY_LENS = [192, 448, 960, 4032]
DECODE_LENS16 = DECODE_LENS + DECODE_BOUNDARY_LENS + [2, 127, 1025]
FLASH_LENS = [1, 63, 64, 65, 127, 128, 129, 200, 385]  # 385: 7 key tiles, more than a three-slot ring
SPIKE_SUPPORT = 16


def pow2ceil(x: float) -> int:
    return 1 << max(0, math.ceil(math.log2(x)))


def dec_chunk(L: int, nsplit: int, chunk: int) -> int:
    """Keys per split of a row of L keys (the kernels' balanced splits)."""
    return min((-(-L // nsplit) + 63) & ~63, chunk)


def mismatches(got, ref, atol=ATOL, rtol=RTOL) -> int:
    """Elements outside the suite's criterion |got - ref| <= atol + rtol |ref| (a NaN is outside)."""
    got, ref = got.float(), ref.float()
    return int((~((got - ref).abs() <= atol + rtol * ref.abs())).sum())


def close(got, ref, what=""):
    got, ref = got.float(), ref.float()
    bad = mismatches(got, ref)
    assert bad == 0, f"{what}: {bad} / {got.numel()} mismatches, max err {(got - ref).abs().max().item():.4g}"


def spike_kappa(beta: float, D: int):
    """(kappa, beta'): the spike key's entries and the score they give against u."""
    x = beta * math.sqrt(D) / 4
    e = math.floor(math.log2(x)) - 3
    kappa = round(x / 2 ** e) * 2 ** e  # 4 significant bits
    return float(kappa), 4 * kappa / math.sqrt(D)


def spike_dir(Hkv: int, D: int):
    """sign pattern [Hkv, D] (+-1 on 16 entries, 0 elsewhere); u = pattern / 4 is a unit vector."""
    s = torch.zeros(Hkv, D)
    i = torch.arange(SPIKE_SUPPORT)
    for hk in range(Hkv):
        s[hk, (i * (D // SPIKE_SUPPORT) + hk) % D] = 1.0 - 2.0 * ((i + hk) % 2)
    return s


def rope_table_90(max_pos: int, D: int, device=None):
    """A RoPE table [max_pos, D/2, 2] whose angles are multiples of 90 degrees (pair i at position p
    turns by 90 p (i + 1)): every rotation is a swap / negation, exact in any format."""
    p = torch.arange(max_pos)[:, None]
    i = torch.arange(D // 2)[None, :]
    t = (p * (i + 1)) % 4
    cos = torch.tensor([1.0, 0.0, -1.0, 0.0])[t]
    sin = torch.tensor([0.0, 1.0, 0.0, -1.0])[t]
    return torch.stack([cos, sin], dim=-1).float().contiguous().to(device)


def _unrotate(x, cs):
    """x [n, heads, D] rotated by MINUS the angles of cs [n, D/2, 2]."""
    x1, x2 = x[..., 0::2], x[..., 1::2]
    c, s = cs[:, None, :, 0], -cs[:, None, :, 1]
    return torch.stack([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).flatten(-2)


def _spike_keys(where, lo, hi):
    """Distinct key indices in [lo, hi) for the named places."""
    if hi <= lo:
        return []
    at = {"first": lo, "middle": (lo + hi) // 2, "last": hi - 1}
    return sorted({at[w] for w in where})


class _Probes:
    """The key <-> (layout, kv head, column) map and the checks shared by both builders."""

    def _init_probes(self, nkeys, rows_keys):
        self.HD = self.Hkv * self.D
        self.n_layouts = max(1, -(-nkeys // self.HD))
        self._want = rows_keys                      # per row: number of keys that must get probed
        self._seen = [np.zeros(n, dtype=bool) for n in rows_keys]

    def _layout_map(self, l):
        f = np.arange(self.HD)
        return l * self.HD + f, ((f // self.D) + l) % self.Hkv, f % self.D  # key, kv head, column

    def _jmap(self, l):
        j, hk, col = self._layout_map(l)
        m = np.empty((self.Hkv, self.D), dtype=np.int64)
        m[hk, col] = j
        return torch.from_numpy(m).to(self.device)

    def assert_covered(self):
        for r, seen in enumerate(self._seen):
            assert seen.all(), f"row {r}: {int((~seen).sum())} of {seen.size} keys never probed"

    def _check(self, ref, inc, what):
        """ref [rows, H*D], inc bool [rows, Hkv, D]: included probes >= 1, everything else exactly 0."""
        r = ref.float().view(ref.shape[0], self.Hkv, self.H // self.Hkv, self.D)
        inc = inc[:, :, None, :].expand_as(r)
        assert bool((r[inc] >= 1.0).all()), f"{what}: an included probe reads below 1.0 in the reference"
        assert bool((r[~inc] == 0).all()), f"{what}: an excluded element is not 0 in the reference"


class DecodeCase(_Probes):
    """Operands of K.decode_attn / R.decode_attn on probe inputs.

    lens: keys per row; row b lives in cache slot b + 1 (slot 0 and everything past a row's 64 probed
    zero keys hold A). pre_P: keys [0, P) of every row with lens >= P (> P with rope) come from the
    prefix slot; the own slot holds A there, and the prefix slot holds A from P on.
    rope: the fused form: q is the qkv row, the new token's k / v (key lens - 1) live there, the cache
    holds A (V) at that key until the call writes it (k_new [B, Hkv, D]: the k row it must write);
    cos_sin is rope_table_90.
    spike = (beta, where): where is a tuple of "first" / "middle" / "last" (of the row's own keys).
    After layout(l): q, k_cache, v_cache, lens, slot, pre (or None), rope (or None) are the call's
    operands (pass clones of q and the caches to a fused-rope call: it writes the cache)."""

    def __init__(self, H, Hkv, D, lens, max_seq=4096, pre_P=0, rope=False, spike=None, device="cpu", seed=0):
        self.H, self.Hkv, self.D, self.max_seq, self.device = H, Hkv, D, max_seq, device
        self.lens_l, self.B = list(lens), len(lens)
        B = self.B
        g = torch.Generator().manual_seed(seed)
        self.slot_l = [b + 1 for b in range(B)]
        self.P_l = [pre_P if (pre_P and L >= pre_P + (1 if rope else 0)) else 0 for L in self.lens_l]
        self.pslot = B + 1
        slots = B + 2
        self.hi_l = [min(L + TILE, max_seq) for L in self.lens_l]
        self._init_probes(max(self.hi_l), self.hi_l)
        self.is_rope = rope
        # ---- keys and queries
        spikes = [[] for _ in range(B)]
        beta1 = 0.0
        sign = spike_dir(Hkv, D)
        if spike is not None:
            kappa, beta1 = spike_kappa(spike[0], D)
            spikes = [_spike_keys(spike[1], P, L) for P, L in zip(self.P_l, self.lens_l)]
        self.spikes = spikes
        nspk = max(len(s) for s in spikes)
        self.A = float(pow2ceil(max(self.lens_l) + nspk * math.exp(beta1)))
        self.k_cache = torch.zeros(slots, Hkv, max_seq, D, dtype=torch.bfloat16, device=device)
        q = torch.zeros(B, H + 2 * Hkv, D)
        if spike is None:
            q[:, :H] = torch.randn(B, H, D, generator=g)
        else:
            q[:, :H] = (sign / 4).repeat_interleave(H // Hkv, 0)[None]
        for b in range(B):
            for j in spikes[b]:
                if rope and j == self.lens_l[b] - 1:
                    q[b, H:H + Hkv] = sign * kappa
                else:
                    self.k_cache[self.slot_l[b], :, j] = (sign * kappa).to(torch.bfloat16).to(device)
        self.rope = None
        self.lens = torch.tensor(self.lens_l, dtype=torch.int32, device=device)
        if rope:
            assert H == Hkv
            cs = rope_table_90(max_seq, D)
            pos = torch.tensor(self.lens_l) - 1
            self.k_new = q[:, H:H + Hkv].to(torch.bfloat16).to(device)  # what the call writes at key lens - 1
            q[:, :H + Hkv] = _unrotate(q[:, :H + Hkv], cs[pos])  # the call's RoPE turns it back, exactly
            self.rope = (cs.to(device), (self.lens - 1).to(torch.int32))
        self.q = q.view(B, -1).to(torch.bfloat16).to(device)
        self.slot = torch.tensor(self.slot_l, dtype=torch.int32, device=device)
        self.pre = None
        if pre_P:
            self.pre = torch.tensor([[P, self.pslot if P else 0] for P in self.P_l], dtype=torch.int32, device=device)
        # ---- V: zero where a correct kernel reads, A everywhere else
        v = torch.full((slots, Hkv, max_seq, D), self.A, dtype=torch.bfloat16, device=device)
        for b in range(B):
            v[self.slot_l[b], :, self.P_l[b]:self.hi_l[b]] = 0
            if rope:
                v[self.slot_l[b], :, self.lens_l[b] - 1] = self.A  # stale: the new token's v is in the qkv row
        if pre_P:
            v[self.pslot, :, :pre_P] = 0
        self.v_cache = v
        self._set = None

    def layout(self, l):
        """Plant layout l's probes (the previous layout's are taken out). Returns inc bool [B, Hkv, D]:
        the probes each row must include."""
        v, A, H, Hkv, D = self.v_cache, self.A, self.H, self.Hkv, self.D
        if self._set is not None:
            v[self._set] = 0
        qv = self.q.view(self.B, H + 2 * Hkv, D)
        qv[:, H + Hkv:] = 0
        j, hk, col = self._layout_map(l)
        S, HK, J, C = [], [], [], []
        for b in range(self.B):
            sel = (j >= self.P_l[b]) & (j < self.hi_l[b])
            self._seen[b][j[sel]] = True
            if self.is_rope:
                new = sel & (j == self.lens_l[b] - 1)
                qv[b, H + Hkv + hk[new], col[new]] = A
                sel &= ~new
            S.append(np.full(int(sel.sum()), self.slot_l[b])); HK.append(hk[sel]); J.append(j[sel]); C.append(col[sel])
        Pmax = max(self.P_l)
        sel = j < Pmax
        for b in range(self.B):
            self._seen[b][j[sel & (j < self.P_l[b])]] = True
        S.append(np.full(int(sel.sum()), self.pslot)); HK.append(hk[sel]); J.append(j[sel]); C.append(col[sel])
        idx = tuple(torch.from_numpy(np.concatenate(x)).to(self.device) for x in (S, HK, J, C))
        v[idx] = A
        self._set = idx
        jm = self._jmap(l)
        return (jm[None] < self.lens[:, None, None].long())

    def check_reference(self, ref, inc, what="decode"):
        self._check(ref, inc, what)


class FlashCase(_Probes):
    """Operands of K.flash_attn_varlen / R.flash_attn_varlen (and the fp16 form) on probe inputs.

    Sequence b's keys are the P prefix keys (cache slot 1 of `cache_k` / `cache_v`, A from P on) and
    its own lens[b]; global key j < P is prefix key j, else own key j - P. from_cache: the own keys
    live in cache slot 2 + b at positions P .., and every other position of that slot holds A.
    spike = (beta, where) with where of "first" / "middle" / "last" (own keys) and "prefix"
    (prefix key P // 2). After layout(l): q / k / v are column views of one packed qkv, prefix and
    kv_cache the optional arguments."""

    def __init__(self, H, Hkv, D, lens, P=0, causal=True, spike=None, dtype=torch.bfloat16, from_cache=False,
                 device="cpu", seed=0):
        self.H, self.Hkv, self.D, self.P, self.causal, self.device = H, Hkv, D, P, causal, device
        self.lens_l, self.B = list(lens), len(lens)
        T = self.T = sum(lens)
        g = torch.Generator().manual_seed(seed)
        self.from_cache = from_cache
        S = self.S = -(-(P + max(lens) + TILE) // TILE) * TILE
        self._init_probes(P + max(lens), [P + L for L in lens])
        cu = np.concatenate([[0], np.cumsum(lens)])
        self.cu_l = cu.tolist()
        self.cu = torch.tensor(self.cu_l, dtype=torch.int32, device=device)
        self.seq_of = np.repeat(np.arange(self.B), lens)
        self.idx_of = np.arange(T) - cu[self.seq_of]
        sign = spike_dir(Hkv, D)
        beta1, nspk, kappa = 0.0, 0, 0.0
        own_sp, pre_sp = [[] for _ in lens], []
        if spike is not None:
            kappa, beta1 = spike_kappa(spike[0], D)
            own_sp = [_spike_keys([w for w in spike[1] if w != "prefix"], 0, L) for L in lens]
            if "prefix" in spike[1] and P:
                pre_sp = [P // 2]
            nspk = max(len(s) for s in own_sp) + len(pre_sp)
        self.A = float(pow2ceil(P + max(lens) + nspk * math.exp(beta1)))
        assert self.A <= torch.finfo(dtype).max
        qkv = torch.zeros(T, H + 2 * Hkv, D)
        if spike is None:
            qkv[:, :H] = torch.randn(T, H, D, generator=g)
        else:
            qkv[:, :H] = (sign / 4).repeat_interleave(H // Hkv, 0)[None]
        for b, sp in enumerate(own_sp):
            for jj in sp:
                qkv[self.cu_l[b] + jj, H:H + Hkv] = sign * kappa
        nslots = 2 + (self.B if from_cache else 0)
        ck = torch.zeros(nslots, Hkv, S, D, dtype=dtype)
        cv = torch.full((nslots, Hkv, S, D), self.A, dtype=dtype)
        cv[1, :, :P] = 0
        for j in pre_sp:
            ck[1, :, j] = (sign * kappa).to(dtype)
        self.kv_cache = None
        if from_cache:
            for b, L in enumerate(lens):
                cv[2 + b, :, P:P + L] = 0
                ck[2 + b, :, P:P + L] = qkv[self.cu_l[b]:self.cu_l[b] + L, H:H + Hkv].transpose(0, 1).to(dtype)
            qkv[:, H:] = 0  # the k / v columns are not the source in this mode
            slot = torch.from_numpy(self.seq_of + 2).to(torch.int32).to(device)
            pos = torch.from_numpy(self.idx_of + P).to(torch.int32).to(device)
        self.cache_k, self.cache_v = ck.to(device), cv.to(device)
        if from_cache:
            self.kv_cache = (self.cache_k, self.cache_v, slot, pos)
        self.prefix = (self.cache_k[1], self.cache_v[1], P) if P else None
        self.qkv = qkv.view(T, -1).to(dtype).to(device)
        self.q = self.qkv[:, :H * D]
        self.k = self.qkv[:, H * D:(H + Hkv) * D]
        self.v = self.qkv[:, (H + Hkv) * D:]
        self.max_len = max(lens)
        self._set = None
        self._i = torch.from_numpy(self.idx_of).to(device)
        self._n = torch.from_numpy(np.asarray(lens)[self.seq_of]).to(device)

    def layout(self, l):
        """Plant layout l's probes. Returns inc bool [T, Hkv, D]: the probes each query must include."""
        A, H, Hkv, D, P = self.A, self.H, self.Hkv, self.D, self.P
        cv = self.cache_v
        if self._set is not None:
            cv[self._set] = 0
        vv = self.qkv.view(self.T, H + 2 * Hkv, D)[:, H + Hkv:]
        vv.zero_()
        j, hk, col = self._layout_map(l)
        S, HK, J, C = [np.full(int((j < P).sum()), 1)], [hk[j < P]], [j[j < P]], [col[j < P]]
        for b, L in enumerate(self.lens_l):
            self._seen[b][j[j < P + L]] = True
            sel = (j >= P) & (j < P + L)
            if self.from_cache:
                S.append(np.full(int(sel.sum()), 2 + b)); HK.append(hk[sel]); J.append(j[sel]); C.append(col[sel])
            else:
                t = torch.from_numpy(self.cu_l[b] + j[sel] - P).to(self.device)
                vv[t, torch.from_numpy(hk[sel]).to(self.device), torch.from_numpy(col[sel]).to(self.device)] = A
        idx = tuple(torch.from_numpy(np.concatenate(x)).to(self.device) for x in (S, HK, J, C))
        cv[idx] = A
        self._set = idx
        jm = self._jmap(l)[None]
        inc = jm < (P + self._n)[:, None, None]
        if self.causal:
            inc = inc & (jm <= (P + self._i)[:, None, None])
        return inc

    def check_reference(self, ref, inc, what="flash"):
        rows = ~torch.isnan(ref.float()[:, 0])  # tail_only: the undefined rows are NaN in the reference
        self._check(ref[rows], inc[rows], what)
