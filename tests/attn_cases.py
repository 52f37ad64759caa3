"""Deterministic inputs for the paged attention kernels whose correct output is known exactly
or to a derived bound, an fp64 reference over the paged layout, and the checkers.

Four input families (``build(family, ...)``), every value exactly representable in bf16:

A  needle     q = beta * K[p]: one key scores >= 20 nats above every other visible key, V
              encodes (token, kv head) in +-1 bits, so the output is exactly V[p]
B  count      q = 0, V one-hot in t % hd: out[d] = (visible tokens with t % hd == d) / visible
C  staircase  the score is constant inside a key tile and steps by about 3 / 5 / 9 (log2 units)
              per tile, up or down; V one-hot in the tile index: each output dim is one tile's
              total weight, so every rescale factor of the online softmax shows
D  random     N(0,1) inputs against the fp64 reference with the bound
              |out - ref| <= 2^-8 * sum_t p_t |v_t| + 2^-7 |ref| + 1e-6

The K/V pool is reached through a shuffled block table.  Block 0, the spare blocks and the
slots past a sequence's end hold NaN, the table is wider than any sequence needs (unused
entries point at block 0) and is a row-strided view: a read of any slot that is not a visible
token of the sequence poisons the output.

Not a test module and not a conftest: ``test_attention_exact_cpu.py`` proves that the checkers
catch one-token, one-page, one-mask-bit and one-rescale slips, ``test_attention_exact_gpu.py``
runs the kernels through them.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Callable, Optional

import torch

from dgi import ops

BF16 = torch.bfloat16
FAMILIES = ("A", "B", "C", "D")
MIN_MARGIN = 20.0                  # nats between the needle and every other visible key
DECODE_TILE, PREFILL_TILE = 32, 64  # keys per online-softmax step of the two kernels
# staircase |q| / |u|: log2 steps of about 3, 5 and 9 per tile (beta * sqrt(hd) / 8 * log2 e)
STAIR_BETAS = {128: (1.5, 2.5, 4.5), 64: (2.0, 3.5, 6.25)}
NEEDLE_BETA = {128: 4.0, 64: 8.0}
# decode split plans of the GPU tests whose part edges the needles probe: (max_splits, -min part)
DEVICE_PLANS = tuple((S, m) for S in (1, 3, 16, 64) for m in (64, 32))


@dataclass
class Case:
    family: str
    nh: int
    nkv: int
    hd: int
    bs: int
    scale: float
    ctxs: list
    qlens: list            # decode: all 1
    causal: bool           # False: decode (every cached key is visible)
    q: torch.Tensor        # [T, (nh + 2 nkv) hd] bf16; columns past nh * hd are NaN
    kc: torch.Tensor       # [blocks, nkv, bs, hd]
    vc: torch.Tensor
    bt: torch.Tensor       # int32 [B, maxw], row stride > maxw
    ctx: torch.Tensor      # int32 [B]
    cu: torch.Tensor       # int32 [B + 1]
    tree_mask: Optional[torch.Tensor] = None
    tree_n: int = 0
    expect: Optional[torch.Tensor] = None      # A: [T, nh, hd] V[needle]
    exact: Optional[torch.Tensor] = None       # A: [T, nh] False = "must not see" row
    needle: Optional[torch.Tensor] = None      # A: [T, nh] key index
    min_margin: float = math.inf               # A: smallest needle margin, nats
    row0: list = field(default_factory=list)   # first output row of each sequence
    ref_cache: Optional[tuple] = None          # reference(c) of the unbroken case

    @property
    def T(self):
        return sum(self.qlens)


@dataclass
class Check:
    ok: bool
    ratio: float      # worst error / tolerance (informational)
    detail: str = ""

    def __bool__(self):
        return self.ok


# ----------------------------------------------------------------------------
# visibility, fp64 reference
# ----------------------------------------------------------------------------

def visible(c: Case, b: int, mutate: Optional[dict] = None) -> torch.Tensor:
    """bool [qlen, ctx]: the keys each query row of sequence b attends to."""
    mutate = mutate or {}
    ql, ctx = c.qlens[b], c.ctxs[b]
    dev = c.kc.device
    if not c.causal:
        return torch.ones(ql, ctx, dtype=torch.bool, device=dev)
    kpos = torch.arange(ctx, device=dev)[None, :]
    qpos = torch.arange(ctx - ql, ctx, device=dev)[:, None]
    allow = (mutate["causal"](kpos, qpos) if "causal" in mutate else kpos <= qpos).clone()
    if c.tree_mask is not None and c.tree_n > 0:
        N = c.tree_n
        bits = [int(x) & ((1 << 64) - 1) for x in c.tree_mask[b, :N].tolist()]
        if "tree_bits" in mutate:
            bits = mutate["tree_bits"](bits)
        if bits is not None:
            m = torch.tensor([[(bits[i] >> a) & 1 for a in range(N)] for i in range(N)], dtype=torch.bool, device=dev)
            allow[ql - N:, ctx - N:] &= m
    return allow


def _gather(c: Case, b: int, mutate: dict):
    ctx = c.ctxs[b]
    nblk = (ctx + c.bs - 1) // c.bs
    ids = c.bt[b, :nblk].long()
    if "block_table" in mutate:
        ids = mutate["block_table"](ids)
    k = c.kc[ids].permute(0, 2, 1, 3).reshape(nblk * c.bs, c.nkv, c.hd)[:ctx].double()
    v = c.vc[ids].permute(0, 2, 1, 3).reshape(nblk * c.bs, c.nkv, c.hd)[:ctx].double()
    if "v_index" in mutate:
        v = v[mutate["v_index"](torch.arange(ctx, device=v.device))]
    return k, v


def _online(s, mult, v, om):
    """Tiled online softmax in fp64, as the kernels run it: tiles of om['tile'] keys, parts of
    om['part'] keys merged by their log-sum-exp.  om may break one step:
    skip_rescale=j (tile j: the max moves, O and l keep the stale scale), alpha_not_l (alpha
    scales O only), equal_splits (parts averaged with equal weights)."""
    H, G, Q, T = s.shape
    W, P = om["tile"], om.get("part") or T
    outs, lses = [], []
    for p0 in range(0, T, P):
        m = torch.full((H, G, Q, 1), -math.inf, dtype=s.dtype, device=s.device)
        l = torch.zeros_like(m)
        o = torch.zeros(H, G, Q, v.shape[-1], dtype=s.dtype, device=s.device)
        for t0 in range(p0, min(p0 + P, T), W):
            t1 = min(t0 + W, p0 + P, T)
            st = s[..., t0:t1]
            m_new = torch.maximum(m, st.amax(-1, keepdim=True))
            dead = torch.isinf(m_new)
            alpha = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp(m - m_new))
            pt = torch.where(dead, torch.zeros_like(st), mult[:, t0:t1] * torch.exp(st - m_new))
            a_o = a_l = alpha
            if om.get("skip_rescale") == t0 // W:
                a_o = a_l = torch.ones_like(alpha)
            if om.get("alpha_not_l"):
                a_l = torch.where(torch.isinf(m), a_l, torch.ones_like(alpha))
            l = l * a_l + pt.sum(-1, keepdim=True)
            o = o * a_o + torch.einsum("hgqt,thd->hgqd", pt, v[t0:t1])
            m = m_new
        outs.append(torch.where(l > 0, o / l, torch.zeros_like(o)))
        lses.append(torch.where(l > 0, m + torch.log(l), torch.full_like(m, -math.inf)))
    lse = torch.stack(lses)                       # [parts, H, G, Q, 1]
    live = ~torch.isinf(lse)
    wgt = torch.where(live, torch.exp(lse - lse.amax(0, keepdim=True)), torch.zeros_like(lse))
    if om.get("equal_splits"):
        wgt = live.to(s.dtype)
    return (wgt * torch.stack(outs)).sum(0) / wgt.sum(0)


def reference(c: Case, mutate: Optional[dict] = None):
    """fp64 attention over the paged pool -> (out, A), both [T, nh * hd] fp64, with
    A = sum_t p_t |v_t| (the scale of family D's rounding bound).

    ``mutate`` breaks the reference for the self-test; hooks by key:
    block_table(ids) -> ids, v_index(t) -> t, causal(kpos, qpos) -> bool, tree_bits(bits) -> bits
    or None (no tree mask), mult(m [qlen, ctx], ctx=) -> m (0 drops a key, 2 counts it twice),
    online = dict for ``_online`` (the tiled form, optionally with one broken rescale).
    """
    mutate = mutate or {}
    if not mutate and c.ref_cache is not None:
        return c.ref_cache
    G = c.nh // c.nkv
    dev = c.kc.device
    out = torch.zeros(c.T, c.nh * c.hd, dtype=torch.float64, device=dev)
    A = torch.zeros_like(out)
    for b, (ql, ctx) in enumerate(zip(c.qlens, c.ctxs)):
        if ql == 0:
            continue
        r0 = c.row0[b]
        k, v = _gather(c, b, mutate)
        qb = c.q[r0:r0 + ql, : c.nh * c.hd].double().view(ql, c.nkv, G, c.hd)
        s = torch.einsum("qhgd,thd->hgqt", qb, k) * c.scale
        mult = visible(c, b, mutate).double()
        if "mult" in mutate:
            mult = mutate["mult"](mult, ctx=ctx)
        s = s.masked_fill((mult == 0)[None, None], -math.inf)
        p = mult * torch.exp(s - s.amax(-1, keepdim=True))
        l = p.sum(-1, keepdim=True)
        p = p / l
        if "online" in mutate:
            o = _online(s, mult, v, mutate["online"]).permute(2, 0, 1, 3)
        else:
            o = torch.einsum("hgqt,thd->qhgd", p, v)
        out[r0:r0 + ql] = o.reshape(ql, -1)
        A[r0:r0 + ql] = torch.einsum("hgqt,thd->qhgd", p, v.abs()).reshape(ql, -1)
    if not mutate:
        c.ref_cache = (out, A)
    return out, A


# ----------------------------------------------------------------------------
# builders
# ----------------------------------------------------------------------------

def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _pm1(gen, *shape):
    return (torch.randint(0, 2, shape, generator=gen) * 2 - 1).to(torch.float32)


def _pack(ktoks, vtoks, bs, dev, gen):
    """Per-sequence [ctx, nkv, hd] tokens -> (k_cache, v_cache, block_tables)."""
    nkv, hd = ktoks[0].shape[1:]
    need = [(k.shape[0] + bs - 1) // bs for k in ktoks]
    nblocks = 1 + sum(need) + 4
    ids = (torch.randperm(nblocks - 1, generator=gen) + 1).tolist()   # block 0 and 4 spares stay NaN
    maxw = max(need) + 5
    store = torch.zeros(len(ktoks), maxw + 3, dtype=torch.int32)
    kp = torch.full((nblocks * bs, nkv, hd), math.nan, dtype=BF16, device=dev)
    vp = torch.full((nblocks * bs, nkv, hd), math.nan, dtype=BF16, device=dev)
    k0 = 0
    for b, n in enumerate(need):
        blk = torch.tensor(ids[k0:k0 + n], dtype=torch.int64)
        store[b, :n] = blk.to(torch.int32)
        k0 += n
        ctx = ktoks[b].shape[0]
        t = torch.arange(ctx, device=dev)
        slot = blk.to(dev)[t // bs] * bs + t % bs
        kp[slot] = ktoks[b].to(dev, BF16)
        vp[slot] = vtoks[b].to(dev, BF16)
    kc = kp.view(nblocks, bs, nkv, hd).permute(0, 2, 1, 3).contiguous()
    vc = vp.view(nblocks, bs, nkv, hd).permute(0, 2, 1, 3).contiguous()
    bt = store.to(dev)[:, :maxw]
    assert bt.stride(0) > bt.shape[1]
    return kc, vc, bt


def part_edges(ctx: int, max_ctx: int, B: int, nkv: int) -> list:
    """First and last token of the first, a middle and the last part of every decode split plan
    the GPU tests drive."""
    plans = [ops.decode_split_plan(B, max_ctx, nkv)[1], 128]
    for S, mn in DEVICE_PLANS:
        ns = max(1, min(S, (ctx + mn - 1) // mn))
        plans.append((((ctx + ns - 1) // ns) + 31) & ~31)
    edges = []
    for part in plans:
        ns = (ctx + part - 1) // part
        for pi in (0, ns // 2, ns - 1):
            edges += [pi * part, min(pi * part + part, ctx) - 1]
    return [e for e in dict.fromkeys(edges) if 0 <= e < ctx]


def decode_needles(ctx: int, n: int, max_ctx: int, B: int, nkv: int, gen) -> list:
    """n needle positions for one decode sequence: 0 and ctx - 1, then split-part edges and both
    sides of the multiples of 128 / 64 / 32 / 16 (as many as fit, in a seeded order), then
    random positions."""
    def shuffled(xs):
        return [xs[i] for i in torch.randperm(len(xs), generator=gen).tolist()]

    cand = [0, ctx - 1] + shuffled(part_edges(ctx, max_ctx, B, nkv))
    seen = set()
    for m in (128, 64, 32, 16):
        sides = [x for t in range(m, ctx, m) if t not in seen for x in (t - 1, t)]
        seen.update(range(m, ctx, m))
        cand += shuffled(sides)
    cand = list(dict.fromkeys(cand))[:n]
    cand += torch.randint(0, ctx, (n - len(cand),), generator=gen).tolist()
    return cand


def _prefill_needles(c_vis, ql, ctx, nh, is_tree):
    """(needle key [ql, nh], exact [ql, nh]) for one prefill sequence.  By (row + head) % 7: key
    0, the row's own position, the one before, the last key of the cached prefix, the 64-key
    tile edge at or below the row and the key before that edge — each only where the row sees
    it, else its own position — and "must not see": the nearest hidden key (a non-ancestor
    below a tree row, else position + 1) where one exists."""
    dev = c_vis.device
    pos = torch.arange(ctx - ql, ctx, device=dev)
    kpos = torch.arange(ctx, device=dev)[None, :]
    edge = pos // PREFILL_TILE * PREFILL_TILE
    hidden_below = ~c_vis & (kpos < pos[:, None]) & is_tree[:, None]
    last_hidden = torch.where(hidden_below.any(1), (hidden_below.long() * kpos).amax(1), pos + 1)
    cand = torch.stack([torch.zeros_like(pos), pos, pos - 1, torch.full_like(pos, ctx - ql - 1), edge, edge - 1,
                        last_hidden], 1)                                    # [ql, 7]
    inb = (cand >= 0) & (cand < ctx)
    seen = c_vis.gather(1, cand.clamp(0, ctx - 1)) & inb
    usable = torch.cat([seen[:, :6], (~seen & inb)[:, 6:]], 1)
    kind = (torch.arange(ql, device=dev)[:, None] + torch.arange(nh, device=dev)[None, :]) % 7
    ok = usable.gather(1, kind)
    needle = torch.where(ok, cand.gather(1, kind), pos[:, None].expand(ql, nh))
    return needle, ~(ok & (kind == 6))


def _v_code(ctx, nkv, hd):
    """V[t, h, :]: t in +-1 bits (dims 0-15), h in +-1 bits (dims 16-23), +1 elsewhere."""
    t = torch.arange(ctx)[:, None, None]
    h = torch.arange(nkv)[None, :, None]
    d = torch.arange(hd)[None, None, :]
    bit = torch.where(d < 16, (t >> d.clamp(max=15)) & 1, torch.where(d < 24, (h >> (d - 16).clamp(0, 7)) & 1, 1))
    return (bit * 2 - 1).to(torch.float32).expand(ctx, nkv, hd).contiguous()


def build(family: str, nh: int, nkv: int, hd: int, ctxs, qlens=None, bs: int = 16, device="cpu",
          tree_mask: Optional[torch.Tensor] = None, tree_n: int = 0, seed: int = 0) -> Case:
    """One launch worth of inputs.  ``qlens=None``: decode (one query row per sequence over its
    whole context); otherwise causal prefill of the last qlens[b] positions of each context,
    the last ``tree_n`` rows under ``tree_mask`` (ops.tree_mask_ref layout)."""
    assert family in FAMILIES and nh % nkv == 0
    dev = torch.device(device)
    gen = _gen(seed * 1000003 + nh * 131 + nkv * 17 + hd)
    causal = qlens is not None
    ctxs = list(ctxs)
    W = PREFILL_TILE if causal else DECODE_TILE
    if family == "C":   # at most hd tiles, so every tile owns one output dim
        ctxs = [min(x, W * hd) for x in ctxs]
    qlens = list(qlens) if causal else [1] * len(ctxs)
    assert all(0 <= ql <= cx and cx >= 1 for ql, cx in zip(qlens, ctxs))
    B, G, T = len(ctxs), nh // nkv, sum(qlens)
    row0 = [sum(qlens[:b]) for b in range(B)]
    kvh = torch.arange(nh) // G
    ktoks, vtoks, qrows = [], [], []
    for b, ctx in enumerate(ctxs):
        ql = qlens[b]
        tile = torch.arange(ctx) // W
        if family == "A":
            k = _pm1(gen, ctx, nkv, hd)
            v = _v_code(ctx, nkv, hd)
            qb = torch.zeros(ql, nh, hd)       # filled below, once the needles are chosen
        elif family == "B":
            k = torch.randn(ctx, nkv, hd, generator=gen)
            v = (torch.arange(hd)[None, None, :] == (torch.arange(ctx) % hd)[:, None, None]).float().expand(ctx, nkv, hd)
            qb = torch.zeros(ql, nh, hd)
        elif family == "C":
            u = _pm1(gen, nkv, hd)
            k = tile[:, None, None].float() * u[None] / 8
            v = (torch.arange(hd)[None, None, :] == (tile % hd)[:, None, None]).float().expand(ctx, nkv, hd)
            var = torch.arange(nh) % 6         # step 3 / 5 / 9 ascending, then descending
            amp = torch.tensor(STAIR_BETAS[hd])[var % 3] * torch.where(var < 3, 1.0, -1.0)
            qb = (amp[:, None] * u[kvh])[None].expand(ql, nh, hd)
        else:
            k = torch.randn(ctx, nkv, hd, generator=gen)
            v = torch.randn(ctx, nkv, hd, generator=gen)
            qb = torch.randn(ql, nh, hd, generator=gen)
        ktoks.append(k)
        vtoks.append(v.contiguous())
        qrows.append(qb)
    kc, vc, bt = _pack(ktoks, vtoks, bs, dev, gen)
    q = torch.full((T, (nh + 2 * nkv) * hd), math.nan, dtype=BF16, device=dev)
    if T:
        q[:, : nh * hd] = torch.cat(qrows).reshape(T, nh * hd).to(dev, BF16)
    c = Case(family, nh, nkv, hd, bs, 1 / math.sqrt(hd), ctxs, qlens, causal, q, kc, vc, bt,
             torch.tensor(ctxs, dtype=torch.int32, device=dev),
             torch.tensor([0] + [r + ql for r, ql in zip(row0, qlens)], dtype=torch.int32, device=dev),
             tree_mask.to(dev) if tree_mask is not None else None, tree_n, row0=row0)
    if family == "A":
        _place_needles(c, ktoks, vtoks, gen)
    return c


def _place_needles(c: Case, ktoks, vtoks, gen):
    dev = c.kc.device
    G = c.nh // c.nkv
    kvh = (torch.arange(c.nh, device=dev) // G)[None, :]
    c.expect = torch.zeros(c.T, c.nh, c.hd, device=dev)
    c.exact = torch.ones(c.T, c.nh, dtype=torch.bool, device=dev)
    c.needle = torch.zeros(c.T, c.nh, dtype=torch.int64, device=dev)
    for b, (ql, ctx) in enumerate(zip(c.qlens, c.ctxs)):
        if ql == 0:
            continue
        rows = slice(c.row0[b], c.row0[b] + ql)
        vis = visible(c, b)
        if c.causal:
            is_tree = torch.arange(ql, device=dev) >= ql - (c.tree_n if c.tree_mask is not None else 0)
            needle, exact = _prefill_needles(vis, ql, ctx, c.nh, is_tree)
        else:
            needle = torch.tensor([decode_needles(ctx, c.nh, max(c.ctxs), len(c.ctxs), c.nkv, gen)], device=dev)
            exact = torch.ones(1, c.nh, dtype=torch.bool, device=dev)
        k, v = ktoks[b].to(dev), vtoks[b].to(dev)
        kn = k[needle, kvh]                                   # [ql, nh, hd]
        c.q[rows, : c.nh * c.hd] = (NEEDLE_BETA[c.hd] * kn).reshape(ql, -1).to(BF16)
        c.expect[rows], c.exact[rows], c.needle[rows] = v[needle, kvh], exact, needle
        # margin of every exact row from the fp64 scores: needle minus the best other visible key
        s = torch.einsum("qnd,tnd->qnt", (NEEDLE_BETA[c.hd] * kn).double(), k[:, kvh[0]].double()) * c.scale
        s = s.masked_fill(~vis[:, None, :], -math.inf)
        top = s.gather(2, needle[..., None]).squeeze(2)
        rest = s.scatter(2, needle[..., None], -math.inf).amax(2)
        margin = (top - rest)[exact]
        assert bool(torch.isfinite(top[exact]).all()), "an exact row's needle is not visible"
        if margin.numel():
            c.min_margin = min(c.min_margin, float(margin.min()))


# ----------------------------------------------------------------------------
# checkers
# ----------------------------------------------------------------------------

def _ratio(err, tol):
    """max err / tol; NaN anywhere, or an error where the tolerance is 0, gives inf."""
    if err.numel() == 0:
        return 0.0
    r = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err == 0, 0.0, math.inf).to(err.dtype))
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    return float(r.max())


def bound_D(ref, A):
    return 2.0 ** -8 * A + 2.0 ** -7 * ref.abs() + 1e-6


def check_A(c: Case, out: torch.Tensor) -> Check:
    """Exact rows: out == V[needle] bit for bit (the needle margin makes every other key's total
    weight < ctx * e^-20 < 1e-4, far below the bf16 half-ulp 2^-9 at 1).  "Must not see" rows:
    within family D's bound of the fp64 reference, and dims 0-15 are not the hidden key's code."""
    assert c.min_margin >= MIN_MARGIN, f"needle margin {c.min_margin:.1f} nats < {MIN_MARGIN}"
    o = out[:, : c.nh * c.hd].double().view(c.T, c.nh, c.hd)
    same = (o == c.expect.double()).all(-1)
    bad_exact = int((~same & c.exact).sum())
    ratio, saw = 0.0, 0
    if not bool(c.exact.all()):
        ref, A = reference(c)
        hid = ~c.exact
        err = (o - ref.view_as(o)).abs()[hid]
        ratio = _ratio(err, bound_D(ref, A).view_as(o)[hid])
        saw = int(((o[..., :16] == c.expect[..., :16].double()).all(-1) & hid).sum())
    ok = bad_exact == 0 and saw == 0 and ratio <= 1.0
    return Check(ok, math.inf if bad_exact or saw else ratio,
                 f"{bad_exact} of {int(c.exact.sum())} needle rows differ from V[needle]; {saw} hidden needles seen; "
                 f"hidden rows at {ratio:.3f} of the bound")


def count_expected(c: Case) -> torch.Tensor:
    """fp64 [T, hd]: n_d / n of every query row, from the visible set alone."""
    dev = c.kc.device
    exp = torch.zeros(c.T, c.hd, dtype=torch.float64, device=dev)
    for b, (ql, ctx) in enumerate(zip(c.qlens, c.ctxs)):
        if ql == 0:
            continue
        vis = visible(c, b).double()
        onehot = (torch.arange(c.hd, device=dev)[None, :] == (torch.arange(ctx, device=dev) % c.hd)[:, None]).double()
        exp[c.row0[b]:c.row0[b] + ql] = (vis @ onehot) / vis.sum(1, keepdim=True)
    return exp


def count_sensitivity(c: Case) -> float:
    """Smallest relative change of a non-zero out[d] when one of its tokens is dropped, in units
    of check_B's tolerance 2^-7: (n - n_d) / (n_d (n - 1)) over rows with n > 1."""
    worst = math.inf
    for b, (ql, ctx) in enumerate(zip(c.qlens, c.ctxs)):
        if ql == 0:
            continue
        vis = visible(c, b).double()
        onehot = (torch.arange(c.hd, device=vis.device)[None, :] == (torch.arange(ctx, device=vis.device) % c.hd)[:, None]).double()
        nd, n = vis @ onehot, vis.sum(1, keepdim=True).expand(ql, c.hd)
        live = (nd > 0) & (n > 1)
        if bool(live.any()):
            worst = min(worst, float(((n - nd) / (nd * (n - 1)))[live].min()) * 2.0 ** 7)
    return worst


def check_B(c: Case, out: torch.Tensor) -> Check:
    """|out - n_d / n| <= 2^-7 n_d / n: bf16 round-to-nearest is at most 2^-8 (every p is exactly
    1 and l an exact integer), one more ulp for the fp32 divide and the split weights."""
    o = out[:, : c.nh * c.hd].double().view(c.T, c.nh, c.hd)
    exp = count_expected(c)[:, None, :].expand_as(o)
    ratio = _ratio((o - exp).abs(), 2.0 ** -7 * exp)
    return Check(ratio <= 1.0, ratio, f"count error at {ratio:.3f} of 2^-7 relative")


def check_C(c: Case, out: torch.Tensor) -> Check:
    """Elements with reference >= 2^-100: relative error <= 2^-6 (two bf16 roundings, P and the
    output, 2^-8 each, doubled for the fp32 exponent arithmetic).  Smaller ones stay small."""
    ref, _ = reference(c)
    o = out[:, : c.nh * c.hd].double()
    big = ref >= 2.0 ** -100
    ratio = _ratio((o - ref).abs()[big], 2.0 ** -6 * ref[big])
    small_ok = bool((o[~big].abs() <= 2.0 ** -99).all())
    return Check(ratio <= 1.0 and small_ok, ratio if small_ok else math.inf,
                 f"tile weights at {ratio:.3f} of 2^-6 relative; underflowed dims small: {small_ok}")


def check_D(c: Case, out: torch.Tensor) -> Check:
    """|out - ref| <= 2^-8 A + 2^-7 |ref| + 1e-6: every P rounded to bf16 in the PV product
    (round to nearest, l summed unrounded), then output rounding plus one ulp."""
    ref, A = reference(c)
    o = out[:, : c.nh * c.hd].double()
    ratio = _ratio((o - ref).abs(), bound_D(ref, A))
    return Check(ratio <= 1.0, ratio, f"random inputs at {ratio:.3f} of the derived bound")


CHECKERS: dict[str, Callable[[Case, torch.Tensor], Check]] = {"A": check_A, "B": check_B, "C": check_C, "D": check_D}


def check(c: Case, out: torch.Tensor) -> Check:
    return CHECKERS[c.family](c, out)
