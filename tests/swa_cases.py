"""Windowed inputs for the paged attention kernels whose correct output is known exactly or to a
derived bound (the sliding-window companion of ``attn_cases``; not a test module).

A query at position p with window W sees keys j with max(0, p - W + 1) <= j <= p.  Three families:

count    q = 0, V one-hot in t % hd: out[d] = (visible tokens with t % hd == d) / visible.  One key
         too many or too few at either edge moves a non-zero output by at least 1 / visible of itself
needle   q = beta * K[t]: by (row + head) % 3 the needle is the row's window start lo (the output must
         be V[lo] bit for bit), lo - 1 (hidden: the output must stay within the random bound of the
         fp64 reference and must not carry that key's code) or the row's own position
random   N(0,1) inputs against the fp64 reference, |out - ref| <= 2^-8 sum p|v| + 2^-7 |ref| + 1e-6

The read contract is poisoned: every K/V slot at a position below ``lo_min & ~63`` is NaN and its
block-table entry points at the NaN block, with ``lo_min`` the lowest window start of the
sequence's query rows.  The pool, the shuffled block table and the NaN spares are ``attn_cases``'s.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

import attn_cases as ac
from dgi import ops

FAMILIES = ("count", "needle", "random")
_AC_FAMILY = {"count": "B", "needle": "A", "random": "D"}
NAN_CODE = 0x7F


@dataclass
class WCase:
    family: str
    window: int
    c: ac.Case                 # q / block table / context lengths (the pool in it is poisoned)
    kc: torch.Tensor           # what the kernel reads: bf16 pages or e4m3 codes
    vc: torch.Tensor
    kv_scale: object           # None or [2, nkv] fp32
    ref: torch.Tensor          # fp64 [T, nh * hd]
    A: torch.Tensor            # fp64 sum_t p_t |v_t|
    expect: object = None      # needle: [T, nh, hd] V[needle]
    exact: object = None       # needle: [T, nh] False = "must not see" row
    count: object = None       # count: fp64 [T, hd]


def visible(ql: int, ctx: int, window: int, dev) -> torch.Tensor:
    """bool [ql, ctx]: j <= p and j > p - W for the last ql positions of a ctx-token sequence."""
    p = torch.arange(ctx - ql, ctx, device=dev)[:, None]
    j = torch.arange(ctx, device=dev)[None, :]
    return (j <= p) & (j > p - window)


def build(family: str, nh: int, nkv: int, hd: int, ctxs, window: int, qlens=None, bs: int = 16, device="cuda",
          fp8: bool = False, seed: int = 0) -> WCase:
    assert family in FAMILIES and window > 0
    c = ac.build(_AC_FAMILY[family], nh, nkv, hd, ctxs, qlens, bs=bs, device=device, seed=seed + window)
    dev = c.kc.device
    G = nh // nkv
    kv_scale = None
    k8 = v8 = None
    if fp8:
        # per-head power-of-two scales; the checks see the dequantised pool, as the kernel does
        h = torch.arange(nkv, device=dev)
        kv_scale = torch.stack([torch.exp2(((h % 3) - 1).float()), torch.exp2((((h + 1) % 3) - 1).float())])
        codes = []
        for j, pool in enumerate((c.kc, c.vc)):
            q8 = ops.quantize_kv_ref(pool.transpose(1, 2), 1.0 / kv_scale[j]).transpose(1, 2).contiguous()
            nan = (q8.view(torch.uint8) & 0x7F) == NAN_CODE
            q8.view(torch.uint8)[nan] = NAN_CODE
            pool.copy_(ops.dequantize_kv_ref(q8.transpose(1, 2), kv_scale[j]).transpose(1, 2).to(torch.bfloat16))
            codes.append(q8)
        k8, v8 = codes
    T = c.T
    ref = torch.zeros(T, nh * hd, dtype=torch.float64, device=dev)
    A = torch.zeros_like(ref)
    w = WCase(family, window, c, c.kc, c.vc, kv_scale, ref, A)
    if family == "needle":
        w.expect = torch.zeros(T, nh, hd, device=dev)
        w.exact = torch.ones(T, nh, dtype=torch.bool, device=dev)
    if family == "count":
        w.count = torch.zeros(T, hd, dtype=torch.float64, device=dev)
    kvh = torch.arange(nh, device=dev) // G
    poison = []
    for b, (ql, ctx) in enumerate(zip(c.qlens, c.ctxs)):
        lo_min = max(0, ctx - ql - window + 1) if ql else ctx      # a sequence without rows reads nothing
        poison.append((lo_min & ~63) // bs)
        if ql == 0:
            continue
        rows = slice(c.row0[b], c.row0[b] + ql)
        k, v = ac._gather(c, b, {})                               # clean [ctx, nkv, hd] fp64
        vis = visible(ql, ctx, window, dev)
        if family == "needle":
            pos = torch.arange(ctx - ql, ctx, device=dev)
            lo = (pos - window + 1).clamp_min(0)
            kind = (torch.arange(ql, device=dev)[:, None] + torch.arange(nh, device=dev)[None, :]) % 3
            hidden = (kind == 1) & (lo[:, None] >= 1)
            needle = torch.where(kind == 0, lo[:, None], torch.where(hidden, lo[:, None] - 1, pos[:, None]))
            kn = k[needle, kvh[None, :]]                          # [ql, nh, hd]
            c.q[rows, : nh * hd] = (ac.NEEDLE_BETA[hd] * kn).reshape(ql, -1).to(torch.bfloat16)
            w.expect[rows] = v[needle, kvh[None, :]].float()
            w.exact[rows] = ~hidden
        qb = c.q[rows, : nh * hd].double().view(ql, nkv, G, hd)
        s = torch.einsum("qhgd,thd->hgqt", qb, k) * c.scale
        s = s.masked_fill(~vis[None, None], -math.inf)
        if family == "needle":
            sq = s.permute(2, 0, 1, 3).reshape(ql, nh, ctx)
            top = sq.gather(2, needle[..., None]).squeeze(2)
            rest = sq.scatter(2, needle[..., None], -math.inf).amax(2)
            ex = w.exact[rows]
            assert bool(torch.isfinite(top[ex]).all()) and not bool(torch.isfinite(top[~ex]).any())
            margin = (top - rest)[ex & torch.isfinite(rest)]
            assert margin.numel() == 0 or float(margin.min()) >= ac.MIN_MARGIN, float(margin.min())
        p = torch.softmax(s, -1)
        ref[rows] = torch.einsum("hgqt,thd->qhgd", p, v).reshape(ql, -1)
        A[rows] = torch.einsum("hgqt,thd->qhgd", p, v.abs()).reshape(ql, -1)
        if family == "count":
            onehot = (torch.arange(hd, device=dev)[None, :] == (torch.arange(ctx, device=dev) % hd)[:, None]).double()
            w.count[rows] = (vis.double() @ onehot) / vis.sum(1, keepdim=True)
    # poison after the references are taken: blocks wholly below lo_min & ~63 become NaN and their
    # table entries point at block 0 (NaN)
    for b, nblk in enumerate(poison):
        if nblk:
            ids = c.bt[b, :nblk].long()
            c.kc[ids] = math.nan
            c.vc[ids] = math.nan
            if fp8:
                k8.view(torch.uint8)[ids] = NAN_CODE
                v8.view(torch.uint8)[ids] = NAN_CODE
            c.bt[b, :nblk] = 0
    assert bool(torch.isnan(c.kc[0]).all())
    if fp8:
        w.kc, w.vc = k8, v8
    return w


def check(w: WCase, out: torch.Tensor) -> ac.Check:
    c = w.c
    o2 = out[:, : c.nh * c.hd].double()
    if w.family == "count":
        o = o2.view(c.T, c.nh, c.hd)
        exp = w.count[:, None, :].expand_as(o)
        ratio = ac._ratio((o - exp).abs(), 2.0 ** -7 * exp)
        return ac.Check(ratio <= 1.0, ratio, f"count error at {ratio:.3f} of 2^-7 relative")
    if w.family == "random":
        ratio = ac._ratio((o2 - w.ref).abs(), ac.bound_D(w.ref, w.A))
        return ac.Check(ratio <= 1.0, ratio, f"random inputs at {ratio:.3f} of the derived bound")
    o = o2.view(c.T, c.nh, c.hd)
    same = (o == w.expect.double()).all(-1)
    bad = int((~same & w.exact).sum())
    hid = ~w.exact
    ratio, saw = 0.0, 0
    if bool(hid.any()):
        err = (o - w.ref.view_as(o)).abs()[hid]
        ratio = ac._ratio(err, ac.bound_D(w.ref, w.A).view_as(o)[hid])
        saw = int(((o[..., :16] == w.expect[..., :16].double()).all(-1) & hid).sum())
    ok = bad == 0 and saw == 0 and ratio <= 1.0
    return ac.Check(ok, math.inf if bad or saw else ratio,
                    f"{bad} of {int(w.exact.sum())} needle rows differ from V[needle]; {saw} hidden needles seen; "
                    f"hidden rows at {ratio:.3f} of the bound")
