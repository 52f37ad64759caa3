"""Kernel entry points: HIP (gfx950) on GPU tensors, pure-torch references on CPU.

Every op has two implementations:

* ``torch.ops.dgi.<op>`` from ``dgi/_C.so`` (hand-written CDNA4 HIP kernels,
  see ``dgi/csrc``) — used whenever the tensors live on the GPU.  If the
  extension is missing on a GPU box the op raises: there is no silent
  eager fallback on the device path.
* ``*_ref`` — a plain PyTorch (fp32 accumulate) version of the same math,
  used for CPU execution (the CPU test-suite, OPT-125m config #1) and as the
  numerics oracle of the kernel tests.
"""
from __future__ import annotations

import math
import os
from typing import Optional

import numpy as np
import torch

from dgi.ops.fp8 import E4M3_MAX, Fp8Weight, quantize_fp8  # noqa: F401  (public: ops.Fp8Weight, ops.quantize_fp8)
from dgi.ops.fp8 import Fp8ExpertWeight, quantize_fp8_experts  # noqa: F401  (public: the MoE experts' container)
from dgi.ops.mxfp4 import Mxfp4Weight, quantize_mxfp4  # noqa: F401  (public: ops.Mxfp4Weight, ops.quantize_mxfp4)

_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "_C.so")
_loaded = False
_load_error: Optional[str] = None


def load_native(required: bool = False) -> bool:
    """Load ``dgi/_C.so`` once. ``required`` raises if it cannot be loaded."""
    global _loaded, _load_error
    if _loaded:
        return True
    if os.path.exists(_LIB):
        try:
            torch.ops.load_library(_LIB)
            _loaded = True
            return True
        except Exception as e:  # pragma: no cover - depends on the box
            _load_error = repr(e)
    else:
        _load_error = f"{_LIB} not built (run `python -m dgi.build`)"
    if required:
        raise RuntimeError(f"dgi native kernels unavailable: {_load_error}")
    return False


_WARNED: set = set()


def _warn_once(key: str, msg: str) -> None:
    if key not in _WARNED:
        _WARNED.add(key)
        import warnings
        warnings.warn(msg, RuntimeWarning, stacklevel=3)


def _call(name: str, *args) -> None:
    """Invoke a dgi HIP op; under DGI_DEBUG_SYNC=1 synchronize and name it on a fault."""
    getattr(torch.ops.dgi, name)(*args)
    if _DEBUG_SYNC:
        from dgi.utils.debug import after_op
        after_op(name, *args)


_DEBUG_SYNC = os.environ.get("DGI_DEBUG_SYNC", "0") == "1"


def native_available() -> bool:
    return load_native(False)


def _native(t: torch.Tensor) -> bool:
    if t.is_cuda:
        load_native(required=True)
        return True
    return False


# ----------------------------------------------------------------------------
# RMSNorm
# ----------------------------------------------------------------------------

def rmsnorm_ref(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    xf = x.float()
    var = xf.pow(2).mean(-1, keepdim=True)
    return (xf * torch.rsqrt(var + eps) * w.float()).to(x.dtype)


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    if _native(x):
        out = torch.empty_like(x) if out is None else out
        _call("rmsnorm", out, x, w, eps)
        return out
    r = rmsnorm_ref(x, w, eps)
    if out is not None:
        out.copy_(r)
        return out
    return r


def fused_add_rmsnorm_ref(x: torch.Tensor, residual: torch.Tensor, w: torch.Tensor, eps: float) -> None:
    s = (x.float() + residual.float()).to(residual.dtype)
    residual.copy_(s)
    x.copy_(rmsnorm_ref(s, w, eps))


def fused_add_rmsnorm(x: torch.Tensor, residual: torch.Tensor, w: torch.Tensor, eps: float) -> None:
    """residual <- x + residual; x <- rmsnorm(residual) * w (in place)."""
    if _native(x):
        _call("fused_add_rmsnorm", x, residual, w, eps)
    else:
        fused_add_rmsnorm_ref(x, residual, w, eps)


# ----------------------------------------------------------------------------
# RoPE + paged cache write
# ----------------------------------------------------------------------------

def rope_cos_sin(head_dim: int, max_pos: int, theta: float, scaling: Optional[dict] = None,
                 device=None) -> torch.Tensor:
    """[max_pos, head_dim] fp32 table: first half cos, second half sin.

    Supports Llama-3.1 style ``rope_scaling`` (``rope_type == "llama3"``).
    """
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float64) / head_dim))
    if scaling and scaling.get("rope_type", scaling.get("type")) == "llama3":
        factor = scaling["factor"]
        lo = scaling.get("low_freq_factor", 1.0)
        hi = scaling.get("high_freq_factor", 4.0)
        old = scaling.get("original_max_position_embeddings", 8192)
        lo_wl, hi_wl = old / lo, old / hi
        wl = 2 * math.pi / inv
        smooth = (old / wl - lo) / (hi - lo)
        scaled = torch.where(wl > lo_wl, inv / factor, inv)
        mid = (1 - smooth) * inv / factor + smooth * inv
        is_mid = (wl <= lo_wl) & (wl >= hi_wl)
        inv = torch.where(is_mid, mid, scaled)
    t = torch.arange(max_pos, dtype=torch.float64)
    f = torch.outer(t, inv)
    return torch.cat([f.cos(), f.sin()], dim=-1).float().to(device)


def _rotate(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    h = x.shape[-1] // 2
    x1, x2 = x[..., :h], x[..., h:]
    return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)


def _rotate_interleaved(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    x1, x2 = x[..., 0::2], x[..., 1::2]
    return torch.stack([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1).flatten(-2)


def _rope(x: torch.Tensor, cs: torch.Tensor, mode: int) -> torch.Tensor:
    """Rotate the first rd = cs.shape[-1] dims of x (fp32); the rest pass through."""
    rd = cs.shape[-1]
    cos, sin = cs[:, None, : rd // 2], cs[:, None, rd // 2:]
    rot = _rotate(x[..., :rd], cos, sin) if mode == 0 else _rotate_interleaved(x[..., :rd], cos, sin)
    return rot if rd == x.shape[-1] else torch.cat([rot, x[..., rd:]], dim=-1)


# ---- fp8 KV cache: pages of OCP e4m3 codes (torch.float8_e4m3fn) with one fp32 scale per
# (K or V, kv head).  ONE definition of the format, used by the references below, by the CPU
# engine and as the oracle of the HIP writer:
#   write: code  = rne_e4m3(clamp(float(x_bf16) * inv_scale, -448, 448)),  inv_scale = 1 / scale (fp32)
#   read:  value = float(code) * scale
KV_FP8 = torch.float8_e4m3fn
KV_FP8_MAX = 448.0


def is_fp8_kv(cache: torch.Tensor) -> bool:
    return cache.dtype == KV_FP8


def quantize_kv_ref(x: torch.Tensor, inv_scale: torch.Tensor) -> torch.Tensor:
    """e4m3 codes of ``x`` [..., n_kv, hd] (or any shape ``inv_scale[:, None]`` broadcasts against).

    ``inv_scale`` is the stored fp32 inverse ``[n_kv]`` (a 0-d tensor or a float also works).
    The clamp is explicit: torch's own cast turns anything past 448 into NaN."""
    inv = torch.as_tensor(inv_scale, dtype=torch.float32, device=x.device)
    if inv.dim() == 1:
        inv = inv[:, None]
    return torch.clamp(x.float() * inv, -KV_FP8_MAX, KV_FP8_MAX).to(KV_FP8)


def dequantize_kv_ref(codes: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """fp32 values of e4m3 ``codes`` [..., n_kv, hd]; ``scale`` is ``[n_kv]`` fp32."""
    sc = torch.as_tensor(scale, dtype=torch.float32, device=codes.device)
    if sc.dim() == 1:
        sc = sc[:, None]
    return codes.float() * sc


def _kv_scale_for(cache: torch.Tensor, scale, what: str):
    """The [2, n_kv] fp32 scale tensor an fp8 cache is used with (ones when none is given);
    None for a bf16 cache, which takes no scales."""
    if not is_fp8_kv(cache):
        if scale is not None:
            raise ValueError(f"{what}: scales given for a {cache.dtype} KV cache")
        return None
    nkv = cache.shape[1]
    if scale is None:
        return torch.ones(2, nkv, dtype=torch.float32, device=cache.device)
    if scale.dtype != torch.float32 or tuple(scale.shape) != (2, nkv):
        raise ValueError(f"{what}: kv scales must be fp32 [2, {nkv}], got {scale.dtype} {tuple(scale.shape)}")
    return scale.contiguous()


def rope_cache_ref(qkv, positions, cos_sin, nh, nkv, hd, slot_mapping, k_cache, v_cache, mode: int = 0,
                   kv_inv_scale=None) -> None:
    T = qkv.shape[0]
    if T == 0:
        return
    bs = k_cache.shape[2]
    cs = cos_sin[positions.long()]
    q = qkv[:, : nh * hd].float().view(T, nh, hd)
    k = qkv[:, nh * hd:(nh + nkv) * hd].float().view(T, nkv, hd)
    v = qkv[:, (nh + nkv) * hd:(nh + 2 * nkv) * hd].view(T, nkv, hd)
    qr = _rope(q, cs, mode).to(qkv.dtype)
    kr = _rope(k, cs, mode).to(qkv.dtype)
    qkv[:, : nh * hd] = qr.reshape(T, nh * hd)
    slots = slot_mapping.long()
    ok = slots >= 0
    if ok.any():
        s = slots[ok]
        blk, off = s // bs, s % bs
        inv = _kv_scale_for(k_cache, kv_inv_scale, "rope_cache")
        if inv is None:
            k_cache[blk, :, off] = kr[ok]
            v_cache[blk, :, off] = v[ok]
        else:
            # the values the bf16 cache would hold (k rounded to the activation dtype), then the quantiser
            k_cache[blk, :, off] = quantize_kv_ref(kr[ok], inv[0])
            v_cache[blk, :, off] = quantize_kv_ref(v[ok], inv[1])


def rope_cache(qkv, positions, cos_sin, nh, nkv, hd, slot_mapping, k_cache, v_cache, mode: int = 0,
               kv_inv_scale=None) -> None:
    """Rotate q in place inside the fused qkv rows, write rotated k and v into the paged cache.

    ``cos_sin`` is [max_pos, rd] (rd <= hd rotary dims); ``mode`` 0 = NeoX
    pairing (Llama, Qwen2), 1 = interleaved pairs (GLM-4, GPT-J).  An fp8 cache
    (``float8_e4m3fn``) is written as e4m3 codes; ``kv_inv_scale`` is the layer's
    stored inverse scales ``[2, n_kv]`` fp32 (``BlockPool.kv_inv_scale[layer]``; ones if None)."""
    if _native(qkv):
        inv = _kv_scale_for(k_cache, kv_inv_scale, "rope_cache")
        _call("rope_cache", qkv, positions, cos_sin, nh, nkv, hd, slot_mapping, k_cache, v_cache, mode, inv)
    else:
        rope_cache_ref(qkv, positions, cos_sin, nh, nkv, hd, slot_mapping, k_cache, v_cache, mode, kv_inv_scale)


def qknorm_rope_cache_ref(qkv, positions, cos_sin, q_gain, k_gain, eps, nh, nkv, hd, slot_mapping, k_cache, v_cache,
                          mode: int = 0, kv_inv_scale=None) -> None:
    """The definition of ``qknorm_rope_cache``: ``rmsnorm_ref`` over every q head (``q_gain``) and
    every k head (``k_gain``), written back into ``qkv``, then ``rope_cache_ref``."""
    T = qkv.shape[0]
    if T == 0:
        return
    q = qkv[:, : nh * hd].view(T, nh, hd)
    k = qkv[:, nh * hd:(nh + nkv) * hd].view(T, nkv, hd)
    qkv[:, : nh * hd] = rmsnorm_ref(q, q_gain, eps).reshape(T, nh * hd)
    qkv[:, nh * hd:(nh + nkv) * hd] = rmsnorm_ref(k, k_gain, eps).reshape(T, nkv * hd)
    rope_cache_ref(qkv, positions, cos_sin, nh, nkv, hd, slot_mapping, k_cache, v_cache, mode, kv_inv_scale)


def qknorm_rope_cache(qkv, positions, cos_sin, q_gain, k_gain, eps, nh, nkv, hd, slot_mapping, k_cache, v_cache,
                      mode: int = 0, kv_inv_scale=None) -> None:
    """``rope_cache`` with a per-head RMSNorm of q and k in front of the rotation (Qwen3):
    every q head is normalised over its ``hd`` dims with the bf16 gain ``q_gain`` ``[hd]``, every
    k head with ``k_gain``, each rounded to the activation dtype as ``rmsnorm`` does, then rotated
    and written as ``rope_cache`` does; v is copied untouched.  The HIP kernel takes NeoX pairing
    (``mode`` 0) over the whole head (``cos_sin`` ``[max_pos, hd]``) with ``hd`` 64 or 128 and
    refuses anything else; the CPU reference is a composition and takes every geometry."""
    if _native(qkv):
        if mode != 0:
            raise ValueError("qknorm_rope_cache: the HIP kernel rotates NeoX pairs only (mode 0), "
                             f"got mode {mode}")
        inv = _kv_scale_for(k_cache, kv_inv_scale, "qknorm_rope_cache")
        _call("qknorm_rope_cache", qkv, positions, cos_sin, q_gain, k_gain, eps, nh, nkv, hd, slot_mapping,
              k_cache, v_cache, inv)
    else:
        qknorm_rope_cache_ref(qkv, positions, cos_sin, q_gain, k_gain, eps, nh, nkv, hd, slot_mapping,
                              k_cache, v_cache, mode, kv_inv_scale)


def qknorm_rope_cache_ok(hd: int, rd: int, mode: int) -> bool:
    """Whether the HIP ``qknorm_rope_cache`` kernel takes this geometry."""
    return hd in (64, 128) and rd == hd and mode == 0


# ----------------------------------------------------------------------------
# Attention
# ----------------------------------------------------------------------------

def _gather_kv(k_cache, v_cache, bt_row, ctx, kv_scale=None):
    """[ctx, n_kv, hd] K and V of one sequence; an fp8 cache comes back dequantised (fp32)."""
    bs = k_cache.shape[2]
    nblk = (ctx + bs - 1) // bs
    ids = bt_row[:nblk].long()
    k = k_cache[ids].permute(0, 2, 1, 3).reshape(nblk * bs, k_cache.shape[1], -1)[:ctx]
    v = v_cache[ids].permute(0, 2, 1, 3).reshape(nblk * bs, v_cache.shape[1], -1)[:ctx]
    sc = _kv_scale_for(k_cache, kv_scale, "paged attention")
    if sc is not None:
        k, v = dequantize_kv_ref(k, sc[0]), dequantize_kv_ref(v, sc[1])
    return k, v


def _check_window(window, what: str) -> int:
    if window < 0:
        raise ValueError(f"{what}: window must be >= 0 (0 = full attention), got {window}")
    return int(window)


def paged_decode_ref(q, k_cache, v_cache, block_tables, context_lens, nh, nkv, scale, kv_scale=None,
                     window: int = 0) -> torch.Tensor:
    """``window > 0``: the row at position ``ctx - 1`` sees the last ``window`` keys only."""
    window = _check_window(window, "paged_decode_ref")
    hd = k_cache.shape[-1]
    B = q.shape[0]
    out = torch.empty(B, nh * hd, dtype=q.dtype, device=q.device)
    G = nh // nkv
    for b in range(B):
        ctx = int(context_lens[b])
        k, v = _gather_kv(k_cache, v_cache, block_tables[b], ctx, kv_scale)
        qb = q[b, : nh * hd].float().view(nkv, G, hd)
        s = torch.einsum("hgd,thd->hgt", qb, k.float()) * scale
        if 0 < window < ctx:
            s[..., : ctx - window] = float("-inf")
        p = torch.softmax(s, dim=-1)
        o = torch.einsum("hgt,thd->hgd", p, v.float())
        out[b] = o.reshape(nh * hd).to(q.dtype)
    return out


def decode_split_plan(batch: int, max_ctx: int, nkv: int, num_cus: int = 256) -> tuple[int, int]:
    """(max_splits, part_size) for the split-KV decode kernel.

    Aim for >= 4 workgroups per CU; part_size is a multiple of 128 tokens
    (4 waves x 32-token tiles)."""
    want = max(1, (4 * num_cus + batch * nkv - 1) // max(1, batch * nkv))
    max_parts = max(1, (max_ctx + 127) // 128)
    splits = min(want, max_parts)
    part = ((max_ctx + splits - 1) // splits + 127) // 128 * 128
    part = max(part, 128)
    splits = (max_ctx + part - 1) // part
    return max(1, splits), part


def paged_decode(q, k_cache, v_cache, block_tables, context_lens, nh, nkv, scale,
                 max_splits: int = 1, part_size: int = 1 << 30, out=None, workspace=None,
                 kv_scale=None, window: int = 0) -> torch.Tensor:
    """Single-token attention for each row of ``q`` over its paged context.

    ``window > 0`` (sliding-window layers): a row sees its last ``window`` keys, its own
    included; the split plan then covers ``[max(0, ctx - window) & ~31, ctx)`` and no K/V slot
    before that is read.  ``window == 0`` launches the unwindowed kernels.

    ``part_size > 0``: fixed parts; ``max_splits``/``part_size`` must cover the
    longest context (``decode_split_plan``).  ``part_size <= 0``: device-side
    plan per sequence — up to ``max_splits`` parts of at least ``-part_size``
    tokens (what captured graphs use).  With ``max_splits > 1`` a workspace
    ``(part_o[B*nh*splits*hd], part_lse[B*nh*splits][, counters[B*nkv] int32 zeros])``
    is used; with counters the last workgroup of each (sequence, kv-head)
    combines the splits (no reduce kernel).  An fp8 cache (``float8_e4m3fn``) is read as
    e4m3 codes times ``kv_scale`` (the layer's ``[2, n_kv]`` fp32 scales; ones if None).
    """
    window = _check_window(window, "paged_decode")
    if _native(q):
        hd = k_cache.shape[-1]
        B = q.shape[0]
        if out is None:
            out = torch.empty(B, nh * hd, dtype=q.dtype, device=q.device)
        cnt = None
        if max_splits > 1:
            if workspace is None:
                workspace = (torch.empty(B * nh * max_splits * hd, dtype=torch.float32, device=q.device),
                             torch.empty(B * nh * max_splits, dtype=torch.float32, device=q.device),
                             torch.zeros(B * nkv, dtype=torch.int32, device=q.device))
            po, pl = workspace[0], workspace[1]
            cnt = workspace[2] if len(workspace) > 2 else None
        else:
            po = pl = torch.empty(0, dtype=torch.float32, device=q.device)
            if part_size > 0:
                part_size = max(128, ((part_size if part_size < (1 << 30) else 1 << 20) + 127) // 128 * 128)
        _call("paged_decode", out, q, k_cache, v_cache, block_tables, context_lens, po, pl,
              nh, nkv, max_splits, part_size, scale, cnt, _kv_scale_for(k_cache, kv_scale, "paged_decode"), window)
        return out
    r = paged_decode_ref(q, k_cache, v_cache, block_tables, context_lens, nh, nkv, scale, kv_scale, window)
    if out is not None:
        out.copy_(r)
        return out
    return r


def paged_prefill_ref(q, k_cache, v_cache, block_tables, cu_seqlens_q, context_lens, nh, nkv, scale,
                      tree_mask=None, tree_n: int = 0, kv_scale=None, window: int = 0) -> torch.Tensor:
    """``window > 0``: the query at position p sees keys j with p - window < j <= p."""
    window = _check_window(window, "paged_prefill_ref")
    if window > 0 and tree_mask is not None and tree_n > 0:
        raise ValueError("paged_prefill_ref: a sliding window cannot be combined with a tree mask")
    hd = k_cache.shape[-1]
    T = q.shape[0]
    out = torch.zeros(T, nh * hd, dtype=q.dtype, device=q.device)
    G = nh // nkv
    cu = cu_seqlens_q.tolist()
    for b in range(len(cu) - 1):
        q0, q1 = cu[b], cu[b + 1]
        ql = q1 - q0
        if ql == 0:
            continue
        ctx = int(context_lens[b])
        k, v = _gather_kv(k_cache, v_cache, block_tables[b], ctx, kv_scale)
        qb = q[q0:q1, : nh * hd].float().view(ql, nkv, G, hd)
        s = torch.einsum("qhgd,thd->hgqt", qb, k.float()) * scale
        qpos = torch.arange(ctx - ql, ctx, device=q.device)
        kpos = torch.arange(ctx, device=q.device)
        allow = kpos[None, :] <= qpos[:, None]
        if 0 < window < ctx:
            allow &= kpos[None, :] > qpos[:, None] - window
        if tree_mask is not None and tree_n > 0:
            tf = ql - tree_n
            key0 = ctx - ql + tf
            bits = tree_mask[b, :tree_n].cpu().tolist()
            for i in range(tree_n):
                m = bits[i] & ((1 << 64) - 1)
                for a in range(tree_n):
                    if key0 + a < ctx and not ((m >> a) & 1):
                        allow[tf + i, key0 + a] = False
        s = s.masked_fill(~allow[None, None], float("-inf"))
        p = torch.softmax(s, dim=-1)
        o = torch.einsum("hgqt,thd->qhgd", p, v.float())
        out[q0:q1] = o.reshape(ql, nh * hd).to(q.dtype)
    return out


# query rows per prefill-attention workgroup: 128 (4 waves) or 256 (8 waves sharing
# each staged K/V tile).  Every producer of ``tiles`` (model runner, EAGLE verify /
# draft metadata, ops.paged_prefill) cuts sequences at this size.
PREFILL_TILE = int(os.environ.get("DGI_PREFILL_TILE", "128"))
# two LDS stages in the prefill attention kernel (one barrier per K/V tile); 0 = the round-4 loop
PREFILL_DB = int(os.environ.get("DGI_PREFILL_DB", "1"))


def order_prefill_tiles(cu_seqlens_q, context_lens=None, tile: int = 0) -> np.ndarray:
    """int32 [n_tiles, 2] (sequence, first query row) of a prefill-attention launch, the
    heaviest tiles first.  A causal tile's work is the keys it reads, kv_end = context -
    qlen + t0 + tile, so in (sequence, row) order the longest workgroups of the last heads
    are dispatched last and run alone at the end of the grid; longest-first ordering lets
    the short ones fill in behind them (the grid is (tiles, heads): every head walks the
    same order).  Ties keep (sequence, row) order.  The estimate is the full-attention one
    for sliding-window layers too: tiles are built once per step for all layers."""
    tile = tile or PREFILL_TILE
    cu = np.asarray(cu_seqlens_q, np.int64)
    nb = len(cu) - 1
    ql = cu[1:] - cu[:-1]
    ctx = ql if context_lens is None else np.asarray(context_lens, np.int64)[:nb]
    seq, t0, work = [], [], []
    for b in range(nb):
        starts = np.arange(0, int(ql[b]), tile, dtype=np.int64)
        seq.append(np.full(len(starts), b, np.int64))
        t0.append(starts)
        work.append(np.minimum(int(ctx[b]), int(ctx[b]) - int(ql[b]) + starts + tile))
    if not seq:
        return np.zeros((0, 2), np.int32)
    seq, t0, work = np.concatenate(seq), np.concatenate(t0), np.concatenate(work)
    order = np.argsort(-work, kind="stable")
    return np.stack([seq[order], t0[order]], 1).astype(np.int32)


def prefill_tiles(cu_seqlens_q: list[int], tile: int = 0, context_lens=None) -> list[tuple[int, int]]:
    return [tuple(t) for t in order_prefill_tiles(cu_seqlens_q, context_lens, tile).tolist()]


def paged_prefill(q, k_cache, v_cache, block_tables, cu_seqlens_q, context_lens, nh, nkv, scale,
                  tiles=None, tree_mask=None, tree_n: int = 0, out=None, kv_scale=None,
                  window: int = 0) -> torch.Tensor:
    """Causal varlen attention of packed queries over the paged KV (prefix + new).  An fp8 cache
    is read as e4m3 codes times ``kv_scale`` (``[2, n_kv]`` fp32; ones if None).  ``window > 0``
    (sliding-window layers): the query at position p sees keys (p - window, p]; no K/V slot before
    the 64-key tile of the sequence's first window start is read; not with a tree mask."""
    window = _check_window(window, "paged_prefill")
    if window > 0 and tree_mask is not None and tree_n > 0:
        raise ValueError("paged_prefill: a sliding window cannot be combined with a tree mask")
    if _native(q) and k_cache.shape[-1] not in (64, 128):
        _warn_once("paged_prefill", f"head_dim {k_cache.shape[-1]}: the MFMA prefill kernel is built for 64 / 128; "
                                    "using the PyTorch reference")
    elif _native(q):
        hd = k_cache.shape[-1]
        if out is None:
            out = torch.empty(q.shape[0], nh * hd, dtype=q.dtype, device=q.device)
        if tiles is None:
            tl = prefill_tiles(cu_seqlens_q.tolist(), context_lens=context_lens.tolist())
            tiles = torch.tensor(tl if tl else [[0, 0]], dtype=torch.int32, device=q.device)[: len(tl)]
        _call("paged_prefill", out, q, k_cache, v_cache, block_tables, cu_seqlens_q, context_lens,
              tiles, nh, nkv, scale, tree_mask, tree_n,
              PREFILL_TILE | ((PREFILL_DB & 1) << 16), _kv_scale_for(k_cache, kv_scale, "paged_prefill"), window)
        return out
    r = paged_prefill_ref(q, k_cache, v_cache, block_tables, cu_seqlens_q, context_lens, nh, nkv, scale,
                          tree_mask, tree_n, kv_scale, window)
    if out is not None:
        out.copy_(r)
        return out
    return r


# ----------------------------------------------------------------------------
# MLP activation
# ----------------------------------------------------------------------------

# ----------------------------------------------------------------------------
# Linear: weight-streaming MFMA kernel for decode-sized M, hipBLASLt otherwise
# ----------------------------------------------------------------------------

# Where the skinny kernel beats hipBLASLt (profiles/r1_skinny_gemm.md, weights
# streamed cold from HBM): K <= 4096 projections of 8B-class models at M <= 8
# (1.3-2.1x on qkv / o / gate_up), and square 4096x4096 (o-proj) up to M = 16
# (at M = 32 the end-to-end decode step was no faster).
# Larger K, the 128k-vocab head and every 70B shape stream at 4.5-5.7 TB/s in
# hipBLASLt already.  DGI_SKINNY_MAX_M=0 disables the kernel.
SKINNY_MAX_M = int(os.environ.get("DGI_SKINNY_MAX_M", "32"))


def _use_skinny(M: int, N: int, K: int) -> bool:
    if M > SKINNY_MAX_M or K % 1024 or N % 16 or K > 4096 or N > 32768:
        return False
    # wide projections (8B gate_up, N = 28672) stay ahead of hipBLASLt up to M = 16
    # with the 16-wave config (profiles/r2_decode8b_fused.md, plain GEMM table)
    return M <= 8 or (N <= 4096 and M <= 16) or (N >= 16384 and M <= 16)


def _env_cfg(name: str, unset: int, table: dict) -> int:
    """A launch-config override from the environment: ``unset`` when absent, else a key of ``table``."""
    cfg = int(os.environ.get(name, str(unset)))
    if cfg != unset and cfg not in table:
        raise ValueError(f"{name}={cfg}: not a launch config of this build, choose from {sorted(table)}")
    return cfg


def _skinny_takes(x: torch.Tensor) -> bool:
    """Whether the weight-streaming kernels (skinny_gemm, _w8, _w4) read this [M, K] activation: bf16 on the
    GPU in 16-byte vectors, rows that do not overlap."""
    return (x.is_cuda and x.dtype == torch.bfloat16 and x.stride(1) == 1 and x.stride(0) % 8 == 0
            and x.data_ptr() % 16 == 0 and (x.shape[0] == 1 or x.stride(0) >= x.shape[1]))


def _skinny_run(op: str, x: torch.Tensor, N: int, out: Optional[torch.Tensor], *args) -> torch.Tensor:
    """``op(r, x, *args)`` for an activation that ``_skinny_takes``: ``r`` is the caller's ``out`` where the
    kernel can write it directly ([M, N] bf16 rows on the GPU), else a fresh buffer copied back."""
    M = x.shape[0]
    load_native(required=True)
    direct = (out is not None and out.dtype == torch.bfloat16 and out.shape == (M, N) and out.is_cuda
              and out.stride(1) == 1 and (M == 1 or out.stride(0) >= N))
    r = out if direct else torch.empty(M, N, dtype=x.dtype, device=x.device)
    _call(op, r, x, *args)
    return r if direct or out is None else out.copy_(r)


def _skinny_cfg_ok(table: dict, default_cfg: int, step: int, cfg: int, N: int, K: int) -> bool:
    """Whether launch config ``cfg`` (0: the default) of a ``table`` over ``step``-deep K steps divides [N, K]."""
    nw, nt, u, _d = table[cfg or default_cfg]
    return K % 1024 == 0 and N % (16 * nt) == 0 and (K // step) % (nw * u) == 0


def _use_skinny_quant(M: int, N: int, K: int) -> bool:
    """The quantised formats take every decode-sized step their kernel can launch."""
    return 0 < M <= min(32, SKINNY_MAX_M) and K % 1024 == 0 and N % 16 == 0


def _dequant(op: str, w, out: Optional[torch.Tensor]) -> torch.Tensor:
    N, K = w.shape
    if out is None or out.numel() < N * K or out.device != w.device or out.dtype != torch.bfloat16:
        out = torch.empty(N * K, dtype=torch.bfloat16, device=w.device)
    out = out.view(-1)[: N * K].view(N, K)
    if w.q.is_cuda:
        load_native(required=True)
        _call(op, out, w.q, w.scale)     # K % 16 (fp8) or % 32 (mxfp4) == 0, checked by the op
    else:
        out.copy_(w.dequant(torch.bfloat16))
    return out


# launch configs of skinny_gemm: cfg -> (waves per workgroup, column tiles per wave, 64-deep K steps
# per load group, ring depth); 0 runs 4.  cfg 5 runs two column tiles at M > 16.  _skinny_cfg selects
# 4 and 5; the others are sweep points (profiles/r1_skinny_gemm.md), of which 3 and 6 are retired.
SKINNY_CFGS = {1: (16, 1, 1, 2), 2: (8, 2, 2, 2), 4: (8, 1, 2, 2), 5: (16, 4, 1, 2),
               7: (8, 1, 1, 4), 8: (8, 1, 2, 4), 9: (4, 1, 2, 4), 10: (4, 1, 1, 8), 11: (8, 1, 1, 8)}
SKINNY_CFG = _env_cfg("DGI_SKINNY_CFG", 0, SKINNY_CFGS)    # > 0 forces a skinny_gemm launch config (sweeps)


def _skinny_cfg(M: int, N: int) -> int:
    if SKINNY_CFG > 0:
        return SKINNY_CFG
    return 5 if (M > 8 and N >= 16384) else 0


# FP8 weight-only projections (skinny_gemm_fp8.hip).  The W8A16 kernel takes every decode-sized
# step it can launch: M <= 32, K % 1024 == 0, N % 16 == 0 — without the bf16 kernel's K <= 4096
# rule, which only marks where hipBLASLt wins and hipBLASLt cannot read this format.  Everything
# else is dequantised to bf16 (dequant_fp8) and runs the bf16 GEMM.
# launch configs of skinny_gemm_w8: cfg -> (waves per workgroup, column tiles per wave, 128-deep
# K steps per load group, ring depth); a config needs N % (16 * tiles) == 0 and
# (K / 128) % (waves * steps) == 0
SKINNY_W8_CFGS = {1: (8, 1, 1, 4), 2: (8, 1, 1, 2), 3: (4, 1, 2, 2), 4: (4, 1, 2, 4), 5: (8, 2, 1, 2),
                  6: (4, 1, 1, 8), 7: (16, 1, 1, 2), 8: (8, 4, 1, 2)}
SKINNY_W8_CFG = _env_cfg("DGI_SKINNY_W8_CFG", 0, SKINNY_W8_CFGS)    # > 0 forces a launch config (sweeps)


def skinny_w8_cfg_ok(cfg: int, N: int, K: int) -> bool:
    """Whether launch config ``cfg`` of ``skinny_gemm_w8`` divides an [N, K] weight."""
    return _skinny_cfg_ok(SKINNY_W8_CFGS, 2, 128, cfg, N, K)


def _skinny_w8_cfg(M: int, N: int) -> int:
    """Launch config per row count and width (profiles/fp8_weights/README.md, weights cold, hipGraph-timed):
    every lane reads its X fragment from L2 whatever M is, so from a few rows on the kernel is bound by
    that traffic and wider column tiles (one X fragment for 2 or 4 weight tiles) win wherever enough
    workgroups remain: N >= 6144 for two tiles, the gate_up widths at M > 8 for four.  Between one and
    two workgroups of two tiles per CU (70B qkv: 320 on 256 CUs) the second round runs a quarter full:
    one tile up to 8 rows, four above."""
    if SKINNY_W8_CFG > 0:
        return SKINNY_W8_CFG
    if M <= 2 or N < 6144 or N % 64:
        return 0
    if 256 < N // 32 < 512:
        return 8 if M > 8 else 0
    return 8 if (M > 8 and N >= 16384) else 5


def linear_fp8_ref(x: torch.Tensor, w: Fp8Weight, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    return torch.nn.functional.linear(x.float(), w.q.float() * w.scale[:, None],
                                      None if bias is None else bias.float()).to(x.dtype)


def dequant_fp8(w: Fp8Weight, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bf16 [N, K] copy of an fp8 weight; ``out``: a flat bf16 buffer of >= N*K elements."""
    return _dequant("dequant_fp8", w, out)


# FP8 W8A8 projections (mfma_gemm_fp8.hip): an opt-in mode on top of the fp8 weights
# (Fp8Weight.act == "fp8").  Steps of at least W8A8_MIN_M rows quantise their activations per
# token (quant_rows_fp8) and multiply e4m3 by e4m3 on the block-scaled MFMA (mfma_gemm_fp8);
# smaller steps keep the W8A16 order below.  A token's numerics therefore depend on the row count
# of the step it runs in.  Default 2048: the smallest measured row count from which quantiser +
# e4m3 GEMM beat dequantise + bf16 GEMM on every Llama-3-8B / 70B projection (the e4m3 kernel has
# one schedule and no split-K, so short steps of the narrow projections lose;
# profiles/w8a8/README.md has the per-shape crossovers: 64 rows for gate_up, 256 for all of 70B).
W8A8_MIN_M = int(os.environ.get("DGI_W8A8_MIN_M", "2048"))


def quant_rows_fp8_ref(x: torch.Tensor):
    """Per-row dynamic e4m3 quantisation of a [M, K] activation, in fp32: ``sx = max|x| / 448`` and
    ``q = rne_e4m3(clamp(x * (448 / max|x|), -448, 448))``; a zero row takes ``sx = 1``."""
    xf = x.float()
    amax = xf.abs().amax(dim=1)
    one = torch.ones_like(amax)
    # tensor / tensor: IEEE divisions (torch turns ``scalar / tensor`` into reciprocal * scalar, and
    # on the GPU ``tensor / scalar`` too — one ulp off often enough to move a code across a tie)
    top = torch.full_like(amax, E4M3_MAX)
    sx = torch.where(amax > 0, amax / top, one)
    inv = torch.where(amax > 0, top / amax, one)
    q = (xf * inv[:, None]).clamp_(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)
    return q, sx


def _quant_rows_native(x: torch.Tensor) -> bool:
    return (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 2 and x.shape[1] % 16 == 0
            and (x.shape[1] <= 1 or x.stride(1) == 1)
            and (x.shape[0] <= 1 or (x.stride(0) >= x.shape[1] and x.stride(0) % 8 == 0))
            and x.data_ptr() % 16 == 0)


def quant_rows_fp8(x: torch.Tensor):
    """``(q, sx)`` of a [M, K] activation: the kernel for bf16 GPU rows, the reference elsewhere."""
    if _quant_rows_native(x):
        load_native(required=True)
        q = torch.empty(x.shape, dtype=torch.float8_e4m3fn, device=x.device)
        sx = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
        _call("quant_rows_fp8", q, sx, x)
        return q, sx
    return quant_rows_fp8_ref(x)


def linear_w8a8_ref(x: torch.Tensor, w: Fp8Weight, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    q, sx = quant_rows_fp8_ref(x)
    r = (q.float() @ w.q.float().T) * sx[:, None] * w.scale[None, :]
    if bias is not None:
        r = r + bias.float()
    return r.to(x.dtype)


def _w8a8_fits(x: torch.Tensor, w: Fp8Weight, bias: Optional[torch.Tensor] = None) -> bool:
    """Whether quant_rows_fp8 + mfma_gemm_fp8 take this activation, weight and bias: shapes, sizes
    and the alignment of their 16-byte (bias: 8-byte) accesses."""
    N, K = w.shape
    return (x.dim() == 2 and x.shape[0] >= 1 and x.shape[1] == K and _quant_rows_native(x)
            and N % 256 == 0 and K % 128 == 0 and K >= 128 and N * K < (1 << 31) and x.shape[0] * K < (1 << 31)
            and w.q.data_ptr() % 16 == 0 and w.scale.data_ptr() % 16 == 0
            and (bias is None or (bias.dtype == torch.bfloat16 and bias.is_contiguous() and bias.data_ptr() % 8 == 0)))


def linear_w8a8(x: torch.Tensor, w: Fp8Weight, bias: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """W8A8 projection of a 2-D activation: quantiser + e4m3 GEMM where the kernels' requirements
    hold, ``linear_w8a8_ref`` otherwise."""
    N = w.shape[0]
    if _w8a8_fits(x, w, bias):
        M = x.shape[0]
        direct = (out is not None and out.dtype == torch.bfloat16 and out.shape == (M, N) and out.is_cuda
                  and out.stride(1) == 1 and (M == 1 or (out.stride(0) >= N and out.stride(0) % 4 == 0))
                  and out.data_ptr() % 8 == 0)
        r = out if direct else torch.empty(M, N, dtype=x.dtype, device=x.device)
        q, sx = quant_rows_fp8(x)
        _call("mfma_gemm_fp8", r, q, sx, w.q, w.scale, bias)
        if direct:
            return out
    else:
        r = linear_w8a8_ref(x, w, bias)
    if out is not None:
        out.copy_(r)
        return out
    return r


def _linear_fp8(x: torch.Tensor, w: Fp8Weight, bias: Optional[torch.Tensor], out: Optional[torch.Tensor]):
    w8a8 = w.act == "fp8" and x.dim() == 2 and x.shape[0] >= W8A8_MIN_M
    if x.dim() == 2 and x.is_cuda and x.dtype == torch.bfloat16:
        M, K = x.shape
        N = w.shape[0]
        if w8a8 and _w8a8_fits(x, w, bias):
            return linear_w8a8(x, w, bias, out)
        if _use_skinny_quant(M, N, K) and _skinny_takes(x):
            return _skinny_run("skinny_gemm_w8", x, N, out, w.q, w.scale, bias, _skinny_w8_cfg(M, N))
        r = torch.nn.functional.linear(x, dequant_fp8(w, w.scratch), bias)
    elif w8a8:
        r = linear_w8a8_ref(x, w, bias)
    else:
        r = linear_fp8_ref(x, w, bias)
    if out is not None:
        out.copy_(r)
        return out
    return r


# MXFP4 weight-only projections (skinny_gemm_mxfp4.hip).  The W4A16 kernel takes every decode-sized
# step it can launch, as the fp8 kernel does: M <= 32, K % 1024 == 0, N % 16 == 0.  Everything else
# is dequantised to bf16 (dequant_mxfp4) and runs the bf16 GEMM.  Every mxfp4 value is a bf16 number,
# so the dequantised weight is exact and both GPU routes multiply the same numbers: a token's result
# depends on the row count only through the summation order (unlike fp8's dequant route, which
# rounds each weight once more).
# launch configs of skinny_gemm_w4: cfg -> (waves per workgroup, column tiles per wave, 256-deep
# K steps per load group, ring depth at M <= 16); a config needs N % (16 * tiles) == 0 and
# (K / 256) % (waves * steps) == 0.  Steps of more than 16 rows run rings of at most two groups
# (one for cfg 8): the X fragment is twice the fp8 kernel's.
SKINNY_W4_CFGS = {1: (4, 1, 1, 4), 2: (4, 1, 1, 2), 3: (8, 1, 1, 2), 4: (8, 1, 1, 4), 5: (4, 2, 1, 2),
                  6: (8, 2, 1, 2), 7: (4, 4, 1, 2), 8: (8, 4, 1, 2)}
SKINNY_W4_CFG = _env_cfg("DGI_SKINNY_W4_CFG", 0, SKINNY_W4_CFGS)    # > 0 forces a launch config (sweeps)


def skinny_w4_cfg_ok(cfg: int, N: int, K: int) -> bool:
    """Whether launch config ``cfg`` of ``skinny_gemm_w4`` divides an [N, K] weight."""
    return _skinny_cfg_ok(SKINNY_W4_CFGS, 2, 256, cfg, N, K)


def _skinny_w4_cfg(M: int, N: int, K: int = 0) -> int:
    """Launch config per row count and shape (profiles/mxfp4_weights/README.md, weights cold,
    hipGraph-timed).  The X fragment is read at twice the fp8 kernel's rate per weight byte, so column
    tiles that share it win earlier than they do for fp8: two tiles per wave (cfg 5) at every row count
    for 6144 <= N < 16384, four (cfg 7; cfg 8 on two row tiles) for the gate_up widths.  The narrow
    projections (N = 4096) keep one tile: 8 waves up to two rows, 4 above.  Between one and two
    workgroups of two tiles per CU (70B qkv: 320 on 256 CUs) one tile up to two rows, four above.
    The 8-wave configs need K % 2048 == 0; ``K`` unknown picks among the 4-wave ones."""
    if SKINNY_W4_CFG > 0:
        return SKINNY_W4_CFG
    k8 = K > 0 and K % 2048 == 0
    one = 3 if (M <= 2 and k8) else 0
    if N < 6144 or N % 64:
        return one
    if N >= 16384 or 256 < N // 32 < 512:
        if N < 16384 and M <= 2:
            return one
        return 8 if (M > 16 and k8) else 7
    return 5


def linear_mxfp4_ref(x: torch.Tensor, w: Mxfp4Weight, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    return torch.nn.functional.linear(x.float(), w.dequant(torch.float32),
                                      None if bias is None else bias.float()).to(x.dtype)


def dequant_mxfp4(w: Mxfp4Weight, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bf16 [N, K] copy of an mxfp4 weight (exact); ``out``: a flat bf16 buffer of >= N*K elements."""
    return _dequant("dequant_mxfp4", w, out)


def _linear_mxfp4(x: torch.Tensor, w: Mxfp4Weight, bias: Optional[torch.Tensor], out: Optional[torch.Tensor]):
    if x.dim() == 2 and x.is_cuda and x.dtype == torch.bfloat16:
        M, K = x.shape
        N = w.shape[0]
        if _use_skinny_quant(M, N, K) and _skinny_takes(x):
            return _skinny_run("skinny_gemm_w4", x, N, out, w.q, w.scale, bias, _skinny_w4_cfg(M, N, K))
        r = torch.nn.functional.linear(x, dequant_mxfp4(w, w.scratch), bias)
    else:
        r = linear_mxfp4_ref(x, w, bias)
    if out is not None:
        out.copy_(r)
        return out
    return r


def linear(x: torch.Tensor, w, bias: Optional[torch.Tensor] = None,
           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = x @ w.T (+ bias) for a 2-D activation; [N, K] weights as stored (bf16 tensor, ``Fp8Weight``
    or ``Mxfp4Weight``)."""
    if isinstance(w, Fp8Weight):
        return _linear_fp8(x, w, bias, out)
    if isinstance(w, Mxfp4Weight):
        return _linear_mxfp4(x, w, bias, out)
    if x.dim() != 2:
        return torch.nn.functional.linear(x, w, bias)
    M, K = x.shape
    N = w.shape[0]
    if (_use_skinny(M, N, K) and _skinny_takes(x) and w.dtype == torch.bfloat16 and w.is_contiguous()
            and w.data_ptr() % 16 == 0):
        return _skinny_run("skinny_gemm", x, N, out, w, bias, _skinny_cfg(M, N))
    r = torch.nn.functional.linear(x, w, bias)
    if out is not None:
        out.copy_(r)
        return out
    return r


# Fused decode GEMM (fused_decode.hip): RMSNorm prologue + SwiGLU / RoPE+KV epilogue.
# Where it pays (profiles/r2_decode8b_fused.md, hipGraph-timed, weights cold):
# the qkv projection at M <= 8 (15 vs 18 us at M = 1 on 8B); gate_up on the persistent
# one-ring workgroups (cfg 12 and 16: X staged once per CU, one weight stream per CU) at every
# M <= 16 (55.5 vs 62.4 us unfused at M = 16, profiles/r3_decode/persistent_gemv.md).
# K <= 4096 (8B-class) like _use_skinny.
# DGI_FUSED_DECODE=0 disables, =force uses it for every M <= 16 and K.
FUSED_DECODE = os.environ.get("DGI_FUSED_DECODE", "1")
FUSED_MAX_M = {"qkv": 8, "gate_up": 16}
# launch configs of fused_skinny: cfg -> (kernel kind, waves per workgroup, 64-deep K steps per
# load group, ring depth).  "two_tile": one workgroup per pair of 16-row tiles; "persistent": one
# workgroup per CU streams 8 + 8 row pair tiles through one ring and stages X once; "quarter": the
# same on 4 + 4 row quarter pairs, which balances 1.5 pair tiles per CU.  The ids are those of the
# sweeps (profiles/r3_decode_gemm/README.md, profiles/r3_decode/persistent_gemv.md, quarter_gemv.md,
# profiles/r5_decode/README.md), whose other points are retired.
FUSED_CFGS = {7: ("two_tile", 8, 1, 4), 12: ("persistent", 8, 1, 8), 16: ("persistent", 16, 1, 4),
              24: ("quarter", 16, 1, 4)}
# Config per projection and row count, the fastest on the 8B shapes, weights cold, hipGraph-timed.
# gate_up + SwiGLU: cfg 16 up to M = 8 (43.0 us at M = 1, 45.5 at 4, 48.2 at 8 against 48.6 / 56.2 /
# 66.1 for the two-tile workgroups), cfg 12 above (16 waves do not fit M = 16's LDS).  qkv + RoPE/KV:
# cfg 24 up to M = 8 (13.16 us at M = 1, 17.40 at 4, 20.23 at 8 against 14.96 / 18.52 / 21.37 for the
# retired one-pair-tile workgroups, profiles/r3_decode/quarter_gemv.md); cfg 7 above, which only DGI_FUSED_DECODE=force reaches (FUSED_MAX_M).
FUSED_M_CFG = {"qkv": ((8, 24), (16, 7)), "gate_up": ((8, 16), (16, 12))}
FUSED_KIND_CFG = {"qkv": _env_cfg("DGI_FUSED_QKV_CFG", -1, FUSED_CFGS),
                  "gate_up": _env_cfg("DGI_FUSED_GU_CFG", -1, FUSED_CFGS)}
FUSED_CFG = _env_cfg("DGI_FUSED_CFG", -1, FUSED_CFGS)      # >= 0 overrides FUSED_KIND_CFG


def fused_cfg(kind: str, M: int) -> int:
    if FUSED_CFG >= 0:
        return FUSED_CFG
    if FUSED_KIND_CFG[kind] >= 0:
        return FUSED_KIND_CFG[kind]
    for m, c in FUSED_M_CFG[kind]:
        if M <= m:
            return c
    return FUSED_M_CFG[kind][-1][1]


def fused_decode_ok(M: int, K: int, kind: str = "qkv") -> bool:
    if FUSED_DECODE == "0" or not 0 < M <= 16 or K % 1024 or M * (K + 8) * 2 > 136 * 1024:
        return False
    if FUSED_DECODE == "force":
        return True
    return K <= 4096 and M <= min(SKINNY_MAX_M, FUSED_MAX_M.get(kind, 0))


def fused_skinny_ref(y, x, res, res_out, gamma, eps, w, bias, pro, epi, positions=None, cos_sin=None,
                     slots=None, k_cache=None, v_cache=None, nh=0, nkv=0):
    """Unfused composition of the same ops (CPU reference / test oracle)."""
    if pro == 2:
        s_ = (x.float() + res.float()).to(x.dtype)
        res_out.copy_(s_)
        xin = s_
    else:
        xin = x
    xn = rmsnorm_ref(xin, gamma, eps) if pro else xin
    out = torch.nn.functional.linear(xn.float(), w.float(), None if bias is None else bias.float()).to(x.dtype)
    if epi == 1:
        out = silu_mul_ref(out)
    elif epi == 2:
        rope_cache_ref(out, positions[: out.shape[0]], cos_sin, nh, nkv, 128, slots[: out.shape[0]], k_cache,
                       v_cache, 0)
    y.copy_(out)
    return y


def fused_skinny(y, x, res, res_out, gamma, eps, w, bias, pro: int, epi: int, positions=None, cos_sin=None,
                 slots=None, k_cache=None, v_cache=None, nh: int = 0, nkv: int = 0, cfg: Optional[int] = None):
    """y = epi(rmsnorm_pro(x [+ res]) @ w.T + bias); pro 2 also writes res_out = x + res.

    epi 0 stores [M, N]; epi 1 is SwiGLU over w = [gate; up] (y is [M, I]);
    epi 2 applies NeoX RoPE to the q/k heads of a fused qkv output and writes k/v
    into the paged cache at ``slots`` (head_dim 128, full rotary; bf16 pages only)."""
    if epi == 2 and k_cache is not None and is_fp8_kv(k_cache):
        raise ValueError("fused_skinny: the RoPE + KV-write epilogue has no fp8 writer; use epi 0 + rope_cache")
    if _native(x):
        if cfg is None:
            cfg = fused_cfg("gate_up" if epi == 1 else "qkv", x.shape[0])
        _call("fused_skinny", y, x, res, res_out, gamma, eps, w, bias, pro, epi, positions, cos_sin, slots,
              k_cache, v_cache, nh, nkv, cfg)
        return y
    return fused_skinny_ref(y, x, res, res_out, gamma, eps, w, bias, pro, epi, positions, cos_sin, slots,
                            k_cache, v_cache, nh, nkv)


# batch-1 decode o-proj (no prologue / epilogue) through the persistent fused GEMV, 16 waves:
# 8.35 vs 8.80 us for the skinny kernel on Llama-3-8B (profiles/r4_decode/plain_proj_fused_configs.json);
# at M >= 2 the skinny kernel is as fast or faster.  DGI_OPROJ_FUSED=0: always ops.linear
OPROJ_FUSED = os.environ.get("DGI_OPROJ_FUSED", "1") == "1"
OPROJ_CFG = 16


def decode_proj(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """A decode step's plain projection (o-proj): the persistent fused GEMV at one row,
    ``linear`` otherwise."""
    M, K = x.shape
    if (OPROJ_FUSED and M == 1 and _native(x) and x.dtype == torch.bfloat16 and x.is_contiguous()
            and w.dtype == torch.bfloat16 and w.is_contiguous() and w.shape[1] == K
            and fused_decode_ok(M, K, "qkv") and w.shape[0] % 16 == 0):
        y = torch.empty(M, w.shape[0], dtype=x.dtype, device=x.device)
        return fused_skinny(y, x, None, None, None, 0.0, w, None, pro=0, epi=0, cfg=OPROJ_CFG)
    return linear(x, w)


_PREFETCH_SINKS: dict = {}


def mall_prefetch(w: torch.Tensor, rows: Optional[torch.Tensor] = None, nrows: int = -1, blocks: int = 256) -> None:
    """Read ``w``'s rows (all, the first ``nrows``, or the int32 ids ``rows``) so that a later
    kernel finds them in the memory-side cache (dgi/csrc/prefetch.hip).  Nothing is written;
    a no-op off the native path."""
    if not _native(w):
        return
    sink = _PREFETCH_SINKS.get(w.device)
    if sink is None:
        sink = _PREFETCH_SINKS[w.device] = torch.zeros(256, dtype=torch.int32, device=w.device)
    _call("mall_prefetch", w, rows, sink, nrows, blocks)


def silu_mul_ref(gu: torch.Tensor) -> torch.Tensor:
    I = gu.shape[-1] // 2
    g = gu[..., :I].float()
    return (torch.nn.functional.silu(g) * gu[..., I:].float()).to(gu.dtype)


def silu_mul(gu: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    if _native(gu):
        if out is None:
            out = torch.empty(*gu.shape[:-1], gu.shape[-1] // 2, dtype=gu.dtype, device=gu.device)
        _call("silu_mul", out, gu)
        return out
    r = silu_mul_ref(gu)
    if out is not None:
        out.copy_(r)
        return out
    return r


def mfma_gemm_ref(x: torch.Tensor, w: torch.Tensor, epi: int = 0) -> torch.Tensor:
    """fp32 reference of ``mfma_gemm``: x @ w.T, or SwiGLU over w = [gate; up]."""
    y = x.float() @ w.float().t()
    if epi == 1:
        I = w.shape[0] // 2
        y = torch.nn.functional.silu(y[:, :I]) * y[:, I:]
    return y.to(x.dtype)


def mfma_gemm_ok(x: torch.Tensor, w: torch.Tensor) -> bool:
    """Shapes/layouts the LDS-tiled MFMA GEMM kernel takes (dgi/csrc/mfma_gemm.hip)."""
    return (x.is_cuda and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and x.dim() == 2
            and x.stride(1) == 1 and x.stride(0) % 8 == 0 and w.is_contiguous() and w.shape[0] % 256 == 0
            and x.shape[1] % 64 == 0 and x.data_ptr() % 16 == 0 and x.shape[0] * x.stride(0) < (1 << 31))


def gemm_split_timeouts(reset: bool = False) -> int:
    """Split-K waits of the MFMA GEMM on the current device that ran out since the last reset
    (the last piece of a tile waits, bounded, for the other pieces' slabs; a timeout means a wrong
    tile).  0 in a healthy process; synchronizes the device.  DGI_DEBUG_SYNC=1 checks it after
    every GEMM."""
    if not native_available() or not torch.cuda.is_available():
        return 0
    return int(torch.ops.dgi.gemm_split_timeouts(bool(reset)))


def mfma_gemm(x: torch.Tensor, w: torch.Tensor, epi: int = 0, out: Optional[torch.Tensor] = None,
              sched: int = 3, streamk: int = 0, phases: int = 0, overlap: bool = True) -> torch.Tensor:
    """Hand-written LDS-tiled MFMA GEMM (256x256 tiles, global_load_lds
    staging, XCD-aware tile order): ``epi`` 0 -> x @ w.T; 1 -> the fused
    SwiGLU of the MLP, silu(x @ gate.T) * (x @ up.T) with w = [gate; up],
    written once (no [M, 2I] intermediate and no separate silu_mul pass).
    ``sched`` 3 is the ping-pong kernel; its ``streamk`` (split-K of the
    last partial wave) policy: 0 auto, 1 off, 2 whenever it applies;
    ``phases`` per K tile: 0 auto (2 up to M = 2560, else 4), 2 or 4;
    ``overlap`` False: no cross-tile prologue / epilogue overlap (A/B).
    ``sched`` 1, or a K that is no multiple of 128 or below 256: the
    simple kernel (one barrier per K step), the bit-exact reference of
    the ping-pong kernel; 0: that kernel in compiler order (kept for
    measurements)."""
    M = x.shape[0]
    N = w.shape[0] // 2 if epi == 1 else w.shape[0]
    if mfma_gemm_ok(x, w):
        load_native(required=True)
        if out is None:
            out = torch.empty(M, N, dtype=x.dtype, device=x.device)
        _call("mfma_gemm", out, x, w, epi, sched, streamk, phases, overlap)
        return out
    r = mfma_gemm_ref(x, w, epi)
    if out is not None:
        out.copy_(r)
        return out
    return r


NORM_RES, NORM_PLAIN, NORM_SWIGLU = 2, 3, 4


def mfma_gemm_norm_ref(x: torch.Tensor, w: torch.Tensor, kind: int, ss: torch.Tensor, eps: float,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 reference of ``mfma_gemm_norm`` (same contract, any device)."""
    y = x.float() @ w.float().t()
    M = x.shape[0]
    if kind == NORM_RES:
        new = (out.float() + y).to(out.dtype)
        out.copy_(new)
        nf = new.float()
        ss[:M, : w.shape[0] // 256].copy_((nf * nf).view(M, -1, 256).sum(-1))
        return out
    rstd = torch.rsqrt(ss[:M].sum(-1, keepdim=True) / x.shape[1] + eps)
    y = y * rstd
    if kind == NORM_SWIGLU:
        I = w.shape[0] // 2
        y = torch.nn.functional.silu(y[:, :I]) * y[:, I:]
    r = y.to(x.dtype)
    if out is None:
        return r
    out.copy_(r)
    return out


def mfma_gemm_norm(x: torch.Tensor, w: torch.Tensor, kind: int, ss: torch.Tensor, eps: float,
                   out: Optional[torch.Tensor] = None, phases: int = 0) -> torch.Tensor:
    """The ping-pong MFMA GEMM with a fused RMSNorm epilogue (dgi/csrc/mfma_gemm.hip, EPI 2-4).

    ``kind`` 2 (NORM_RES): ``out`` is the residual stream, updated in place to out + x @ w.T,
    and ``ss[m, j]`` receives the sum of squares of the new row m over columns 256 j .. 256 j + 255
    (``ss`` has at least N / 256 columns; the consumers read a multiple of 8 <= 32, extra
    columns zero): the statistics of the next RMSNorm, with no norm kernel.
    ``kind`` 3 / 4 (NORM_PLAIN / NORM_SWIGLU): x is the un-normalised residual stream and
    ``w`` carries the norm's gain (``LlamaModel.fold_norms``); each output row is scaled by
    rsqrt(sum(ss[m]) / K + eps) — then SwiGLU for kind 4 — which equals
    (rmsnorm(x) * gamma) @ w.T up to rounding."""
    M = x.shape[0]
    N = w.shape[0] // 2 if kind == NORM_SWIGLU else w.shape[0]
    if kind == NORM_RES and out is None:
        raise ValueError("mfma_gemm_norm: kind 2 updates the residual `out` in place")
    if _native(x):
        if out is None:
            out = torch.empty(M, N, dtype=x.dtype, device=x.device)
        _call("mfma_gemm_norm", out, x, w, kind, ss, 1.0 / x.shape[1], eps, phases)
        return out
    return mfma_gemm_norm_ref(x, w, kind, ss, eps, out)


def mfma_gemm_norm_rope_ref(x, w, ss, eps, positions, cos_sin, slots, k_cache, v_cache, nh, nkv,
                            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 reference of ``mfma_gemm_norm_rope``: the normalised qkv (bf16), then RoPE + paged KV
    write (``rope_cache_ref``, NeoX, head dim 128)."""
    y = mfma_gemm_norm_ref(x, w, NORM_PLAIN, ss, eps)
    rope_cache_ref(y, positions[: x.shape[0]], cos_sin, nh, nkv, 128, slots[: x.shape[0]], k_cache, v_cache, 0)
    if out is None:
        return y
    out.copy_(y)
    return out


def mfma_gemm_norm_rope(x, w, ss, eps, positions, cos_sin, slots, k_cache, v_cache, nh: int, nkv: int,
                        out: Optional[torch.Tensor] = None, phases: int = 0) -> torch.Tensor:
    """The normalised qkv projection with RoPE and the paged-KV write in its epilogue
    (mfma_gemm.hip EPI 5): returns y whose q columns are rotated (its k / v columns are NOT
    written — they go to ``k_cache`` / ``v_cache`` at ``slots``, which attention reads), i.e.
    ``mfma_gemm_norm(x, w, NORM_PLAIN, ss)`` followed by ``rope_cache`` in one kernel.  Llama
    geometry: head dim 128, full NeoX rotary, cos_sin [max_pos, 128]; bf16 pages only."""
    if is_fp8_kv(k_cache):
        raise ValueError("mfma_gemm_norm_rope: no fp8 KV writer; use mfma_gemm_norm + rope_cache")
    if _native(x):
        if out is None:
            out = torch.empty(x.shape[0], w.shape[0], dtype=x.dtype, device=x.device)
        _call("mfma_gemm_norm_rope", out, x, w, ss, 1.0 / x.shape[1], eps, positions, cos_sin, slots, k_cache,
              v_cache, nh, nkv, phases)
        return out
    return mfma_gemm_norm_rope_ref(x, w, ss, eps, positions, cos_sin, slots, k_cache, v_cache, nh, nkv, out)


def mfma_norm_ok(x: torch.Tensor, w: torch.Tensor) -> bool:
    """Shapes the fused-norm GEMM takes (K % 128 and >= 256 on top of ``mfma_gemm_ok``; a
    normalising consumer also needs its K — the stream width — <= 8192: 32 row partials)."""
    return mfma_gemm_ok(x, w) and x.shape[1] % 128 == 0 and x.shape[1] >= 256


def row_sumsq(x: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out[:, 0] = sum of squares of each row of x (fp32), the other columns zero: the
    statistics the fused-norm GEMM reads for a stream no residual epilogue produced (the
    first layer's input)."""
    out.zero_()
    xf = x.float()
    out[: x.shape[0], 0] = (xf * xf).sum(-1)
    return out


# ----------------------------------------------------------------------------
# Sampling
# ----------------------------------------------------------------------------

def topkp_threshold(logits: torch.Tensor, temperature: torch.Tensor, top_k: torch.Tensor,
                    top_p: torch.Tensor) -> torch.Tensor:
    """Per-row logit cut for top-k / top-p: keep ``logits >= thresh`` (fp32 [B]).

    HF / vLLM order (temperature, then top-k, then nucleus over the top-k
    survivors, renormalised): element v is kept iff ``#{u > v} < top_k`` and
    ``sum_{u > v} exp(u / T) <= top_p * Z_k`` where ``Z_k`` is the softmax mass of
    the top-k set.  Ties at the cut are kept.  Rows that are greedy (T <= 1e-5)
    or unfiltered (top_k <= 0 and top_p >= 1) get -inf.  Native path: one HIP
    kernel (sampler.hip, interval searches with register-resident counters; no
    sort)."""
    B, V = logits.shape
    if _native(logits):
        th = torch.empty(B, dtype=torch.float32, device=logits.device)
        _call("topkp_threshold", th, logits, temperature.float().contiguous(), top_k.long().contiguous(),
                                      top_p.float().contiguous())
        return th
    lf = logits.float()
    s, _ = lf.sort(dim=-1, descending=True)
    t = temperature.float().clamp(min=1e-5)[:, None]
    fin = torch.isfinite(s)
    e = torch.where(fin, torch.exp((s - s[:, :1]) / t), torch.zeros_like(s))
    cum_excl = e.cumsum(-1) - e
    asc = s.flip(-1).contiguous()
    cnt_gt = V - torch.searchsorted(asc, s, right=True)              # #{u > v}
    mass_gt = cum_excl.gather(-1, cnt_gt.clamp(max=V - 1))           # sum over u > v
    k = torch.where(top_k > 0, top_k.long().clamp(max=V), torch.full_like(top_k.long(), V))
    in_k = (cnt_gt < k[:, None]) & fin
    z_k = torch.where(in_k, e, torch.zeros_like(e)).sum(-1, keepdim=True)   # mass of the top-k survivors
    ok = in_k & (mass_gt <= top_p.float()[:, None] * z_k)
    last = ok.sum(-1) - 1                                            # kept prefix of the sorted row
    th = s.gather(-1, last.clamp(min=0)[:, None]).squeeze(-1)
    keep_all = ok.sum(-1) == fin.sum(-1)                             # every finite logit survives
    off = (temperature <= 1e-5) | ((top_k <= 0) & (top_p >= 1.0)) | keep_all
    return torch.where(off.to(th.device), torch.full_like(th, float("-inf")), th)


def apply_top_k_top_p(logits: torch.Tensor, top_k: torch.Tensor, top_p: torch.Tensor,
                      temperature: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Mask (to -inf) the logits outside the top-k / top-p set (see ``topkp_threshold``)."""
    if temperature is None:
        temperature = torch.ones(logits.shape[0], device=logits.device)
    th = topkp_threshold(logits, temperature, top_k, top_p)
    lf = logits.float()
    return lf.masked_fill(lf < th[:, None], float("-inf"))


_M32 = 0xFFFFFFFF


def _hash32(x: torch.Tensor) -> torch.Tensor:
    """sampler.hip ``hash32`` on int64 tensors holding uint32 values (products
    wrap mod 2^64, so the low 32 bits are exact)."""
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & _M32
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & _M32
    return x ^ (x >> 16)


def gumbel_uniform(seeds: Optional[torch.Tensor], step: int, V: int, B: int) -> torch.Tensor:
    """The per-(row, vocab id) uniforms the HIP sampler draws: a counter-based
    hash of (row seed, step, token id), so a row's draw depends on its own seed
    only (never on the batch it shares) and CPU and GPU pick the same tokens."""
    sd = seeds.long().cpu() if seeds is not None else torch.zeros(B, dtype=torch.long)
    row = ((sd * 2654435761) & _M32) ^ ((step * 40503) & _M32)
    ids = _hash32((torch.arange(V, dtype=torch.long) + 0x9E3779B9) & _M32)
    h = _hash32(row[:, None] ^ ids[None, :])
    return ((h >> 8).float() + 0.5) * (1.0 / 16777216.0)


def sample(logits: torch.Tensor, temperature: Optional[torch.Tensor] = None,
           seeds: Optional[torch.Tensor] = None, step: int = 0, out: Optional[torch.Tensor] = None,
           top_k: Optional[torch.Tensor] = None, top_p: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Greedy (temperature 0) or Gumbel-max sampling per row; returns int64 token ids.

    With ``top_k`` / ``top_p`` the draw is restricted to ``topkp_threshold``'s set
    (on GPU: a threshold kernel + the threshold-aware sampler, no sort and no
    masked copy of the logits)."""
    B = logits.shape[0]
    filt = top_k is not None and top_p is not None and temperature is not None
    if _native(logits):
        if out is None:
            out = torch.empty(B, dtype=torch.long, device=logits.device)
        th = topkp_threshold(logits, temperature, top_k, top_p) if filt else None
        _call("sample", out, logits, temperature, seeds, step, th)
        return out
    if filt:
        logits = apply_top_k_top_p(logits, top_k, top_p, temperature)
    lf = logits.float()
    if temperature is None or bool((temperature <= 1e-5).all()):
        r = lf.argmax(-1)
    else:
        t = temperature.float().clamp(min=1e-5)
        noisy = lf / t[:, None] - torch.log(-torch.log(gumbel_uniform(seeds, step, lf.shape[1], B)))
        r = torch.where(temperature <= 1e-5, lf.argmax(-1), noisy.argmax(-1))
    if out is not None:
        out.copy_(r)
        return out
    return r


def topk_logprobs(logits: torch.Tensor, k: int):
    """Top-k (k <= 16) of ``log_softmax(logits.float())`` per row: fp32 log-probs and int64
    indices, descending (ties: lower index first).  Native path (k <= 8): two HIP kernels
    straight from bf16 logits (sampler.hip: chunked top-k + logsumexp, then a per-row merge)."""
    if _native(logits) and logits.dtype == torch.bfloat16 and logits.stride(-1) == 1 \
            and logits.stride(0) % 8 == 0 and k <= 8:
        B = logits.shape[0]
        v = torch.empty(B, k, dtype=torch.float32, device=logits.device)
        i = torch.empty(B, k, dtype=torch.long, device=logits.device)
        _call("topk_logprobs", v, i, logits, k)
        return v, i
    return topk(torch.log_softmax(logits.float(), dim=-1), k)


def topk(logits: torch.Tensor, k: int):
    """Top-k (k <= 16) values (fp32) and indices (int64), descending."""
    if _native(logits):
        B = logits.shape[0]
        v = torch.empty(B, k, dtype=torch.float32, device=logits.device)
        i = torch.empty(B, k, dtype=torch.long, device=logits.device)
        _call("topk", v, i, logits, k)
        return v, i
    v, i = logits.float().topk(k, dim=-1)
    return v, i


# ----------------------------------------------------------------------------
# Mixture of experts (moe.hip): router, expert-sorted layout, grouped GEMM, combine
# ----------------------------------------------------------------------------
# A token's k experts occupy the flat slots t*k + j (j in descending logit order).  The sorted
# layout groups the slots by expert, ascending slot inside an expert, each expert padded to the
# grouped GEMM's row block BM; P rows hold any assignment of n slots to E experts.
MOE_MAX_EXPERTS = 256
MOE_MAX_TOPK = 16
MOE_EPI_PLAIN, MOE_EPI_SWIGLU = 0, 1


def moe_capacity(n: int, E: int, BM: int) -> int:
    """Rows of the sorted layout of ``n`` slots over ``E`` experts with row blocks of ``BM``."""
    return BM * ((n + BM - 1) // BM + min(E, n))


def moe_block_rows(T: int, k: int, E: int) -> int:
    """Row block of the grouped GEMM for a step: 32 once an expert averages more than 16 rows."""
    return 32 if T * k > 16 * E else 16


def _route_weights(logits: torch.Tensor, ids: torch.Tensor, norm: bool) -> torch.Tensor:
    """fp32 softmax probabilities of ``logits`` at ``ids``: exp(l - max) over the chosen sum
    (``norm``) or over the full sum."""
    lf = logits.float()
    m = lf.max(-1, keepdim=True).values
    p = torch.exp(lf.gather(-1, ids.long()) - m)
    den = p.sum(-1, keepdim=True) if norm else torch.exp(lf - m).sum(-1, keepdim=True)
    return p / den


def moe_route_ref(logits: torch.Tensor, k: int, norm: bool):
    """The definition of ``moe_route``: the k largest LOGITS per row in descending order, ties to
    the lower expert index (a stable sort), and their fp32 softmax weights."""
    order = torch.sort(-logits.float(), dim=-1, stable=True).indices
    ids = order[:, :k].to(torch.int32)
    return ids, _route_weights(logits, ids, norm)


def _moe_route_native(logits: torch.Tensor, k: int) -> bool:
    E = logits.shape[-1]
    return (logits.is_cuda and logits.dim() == 2 and logits.dtype in (torch.bfloat16, torch.float32)
            and logits.stride(1) == 1 and E <= MOE_MAX_EXPERTS and 1 <= k <= min(E, MOE_MAX_TOPK))


def moe_route(logits: torch.Tensor, k: int, norm: bool):
    """Router logits ``[T, E]`` (bf16 or fp32) -> ``ids [T, k]`` int32, ``weights [T, k]`` fp32."""
    if not 1 <= k <= logits.shape[-1]:
        raise ValueError(f"moe_route: k={k} outside 1..E={logits.shape[-1]}")
    if _moe_route_native(logits, k) and logits.shape[0] > 0:
        load_native(required=True)
        T = logits.shape[0]
        ids = torch.empty(T, k, dtype=torch.int32, device=logits.device)
        w = torch.empty(T, k, dtype=torch.float32, device=logits.device)
        _call("moe_route", ids, w, logits, k, bool(norm))
        return ids, w
    return moe_route_ref(logits, k, norm)


def moe_align_ref(ids: torch.Tensor, E: int, BM: int):
    """The definition of ``moe_align``: (counts [E], offsets [E + 1], sorted_slot [P],
    block_expert [P / BM], inv [n]), all int32.  Slots are grouped by expert in ascending slot
    order (a stable sort), expert e starts at the BM-padded ``offsets[e]``; padding rows and the
    unused tail hold -1."""
    flat = ids.reshape(-1).long()
    n = flat.numel()
    P = moe_capacity(n, E, BM)
    dev = flat.device
    counts = torch.bincount(flat, minlength=E)[:E]
    padded = (counts + BM - 1) // BM * BM
    ends = torch.cumsum(padded, 0)
    offsets = torch.cat([ends.new_zeros(1), ends])
    order = torch.sort(flat, stable=True).indices            # slots by expert, ascending inside one
    first = torch.cumsum(counts, 0) - counts                  # unpadded start of each expert
    ex = flat[order]
    pos = offsets[ex] + (torch.arange(n, device=dev) - first[ex])
    sorted_slot = torch.full((P,), -1, dtype=torch.int32, device=dev)
    sorted_slot[pos] = order.to(torch.int32)
    inv = torch.empty(n, dtype=torch.int32, device=dev)
    inv[order] = pos.to(torch.int32)
    be = torch.searchsorted(ends, torch.arange(P // BM, device=dev) * BM, right=True)
    block_expert = torch.where(be < E, be, torch.full_like(be, -1)).to(torch.int32)
    return counts.to(torch.int32), offsets.to(torch.int32), sorted_slot, block_expert, inv


def moe_align(ids: torch.Tensor, E: int, BM: int):
    """Expert-sorted layout of the routing ``ids`` (int32, ``[T, k]`` or flat); see ``moe_align_ref``."""
    if BM not in (16, 32):
        raise ValueError(f"moe_align: BM must be 16 or 32, got {BM}")
    if ids.is_cuda and ids.dtype == torch.int32 and E <= MOE_MAX_EXPERTS and ids.numel() > 0:
        load_native(required=True)
        flat = ids.reshape(-1).contiguous()
        n = flat.numel()
        P = moe_capacity(n, E, BM)
        mk = lambda m: torch.empty(m, dtype=torch.int32, device=ids.device)     # noqa: E731
        counts, offsets, sorted_slot, block_expert, inv = mk(E), mk(E + 1), mk(P), mk(P // BM), mk(n)
        _call("moe_align", counts, offsets, sorted_slot, block_expert, inv, flat, E, BM)
        return counts, offsets, sorted_slot, block_expert, inv
    return moe_align_ref(ids, E, BM)


def _silu_mul_f32(gu: torch.Tensor) -> torch.Tensor:
    I = gu.shape[-1] // 2
    return torch.nn.functional.silu(gu[..., :I]) * gu[..., I:]


def _expert_f32(w, e: int) -> torch.Tensor:
    """Expert ``e`` of ``w`` ([E, N, K] tensor or ``Fp8ExpertWeight``) in fp32; the container is
    dequantised as ``linear_fp8_ref`` does (``q.float() * scale[:, None]``)."""
    return w[e].dequant(torch.float32) if isinstance(w, Fp8ExpertWeight) else w[e].float()


def _expert_pair_quantised(gate_up, down) -> bool:
    """Whether the block's experts are ``Fp8ExpertWeight``: both, or neither."""
    qg, qd = isinstance(gate_up, Fp8ExpertWeight), isinstance(down, Fp8ExpertWeight)
    if qg != qd:
        raise ValueError("moe_mlp: gate_up and down must both be Fp8ExpertWeight or both be tensors, got "
                         f"{type(gate_up).__name__} and {type(down).__name__}")
    return qg


def moe_gemm_ref(x: torch.Tensor, w, sorted_slot: torch.Tensor, block_expert: torch.Tensor, k: int,
                 epi: int, BM: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The definition of ``moe_gemm``: row p of row block b is ``A[p] · w[block_expert[b]]^T`` with
    fp32 accumulation, rounded once to ``x.dtype``; an ``Fp8ExpertWeight`` is dequantised per expert
    (``q.float() * scale[:, None]``).  SwiGLU (``epi`` 1, ``w = [gate; up]``): A[p] is
    token ``sorted_slot[p] // k`` of ``x`` and the fp32 ``silu(gate) * up`` is what is rounded; plain:
    A[p] is row p of ``x``.  Padding rows (slot -1) are left as ``out`` had them (zeros without ``out``)."""
    P = sorted_slot.numel()
    N = w.shape[1] // 2 if epi else w.shape[1]
    if out is None:
        out = torch.zeros(P, N, dtype=x.dtype, device=x.device)
    row_e = block_expert.long().repeat_interleave(BM)
    slot = sorted_slot.long()
    for e in torch.unique(row_e[slot >= 0]).tolist():
        rows = torch.nonzero((row_e == e) & (slot >= 0)).flatten()
        a = x[slot[rows] // k] if epi else x[rows]
        y = a.float() @ _expert_f32(w, e).t()
        out[rows] = (_silu_mul_f32(y) if epi else y).to(out.dtype)
    return out


def _moe_gemm_native(x: torch.Tensor, w: torch.Tensor, epi: int) -> bool:
    N = w.shape[1] // 2 if epi else w.shape[1]
    return (x.is_cuda and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and x.dim() == 2 and w.dim() == 3
            and x.stride(1) == 1 and x.stride(0) % 8 == 0 and w.is_contiguous() and x.shape[1] % 256 == 0
            and N % 16 == 0 and w.shape[0] <= MOE_MAX_EXPERTS and x.data_ptr() % 16 == 0)


def _moe_gemm_w8_native(x: torch.Tensor, w: Fp8ExpertWeight, epi: int) -> bool:
    N = w.shape[1] // 2 if epi else w.shape[1]
    return (x.is_cuda and w.q.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 2 and x.stride(1) == 1
            and x.stride(0) % 8 == 0 and x.shape[1] % 256 == 0 and x.shape[1] == w.shape[2] and N % 16 == 0
            and w.shape[0] <= MOE_MAX_EXPERTS and x.data_ptr() % 16 == 0 and w.q.data_ptr() % 16 == 0
            and w.scale.data_ptr() % 16 == 0)


def moe_gemm(x: torch.Tensor, w, sorted_slot: torch.Tensor, block_expert: torch.Tensor, k: int,
             epi: int, BM: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Grouped GEMM over the sorted layout (``moe_align``): ``[P, N]`` in sorted order.  ``epi``
    ``MOE_EPI_SWIGLU`` gathers token rows of ``x [T, K]`` and applies SwiGLU over ``w [E, 2N, K]``;
    ``MOE_EPI_PLAIN`` reads ``x [P, K]`` in sorted order against ``w [E, N, K]``.  ``k`` is the experts
    per token (the slot -> token divisor).  The HIP kernel takes bf16, K % 256 == 0, N % 16 == 0.
    ``w`` may be an ``Fp8ExpertWeight`` (``moe_gemm_w8``: e4m3 codes, per-expert per-channel scales)."""
    if isinstance(w, Fp8ExpertWeight):
        if not _moe_gemm_w8_native(x, w, epi):
            return moe_gemm_ref(x, w, sorted_slot, block_expert, k, epi, BM, out)
        load_native(required=True)
        P = sorted_slot.numel()
        N = w.shape[1] // 2 if epi else w.shape[1]
        if out is None:
            out = torch.empty(P, N, dtype=x.dtype, device=x.device)
        nslots = x.shape[0] * k if epi else P
        _call("moe_gemm_w8", out, x, w.q, w.scale, sorted_slot, block_expert, k, nslots, epi, BM)
        return out
    if _moe_gemm_native(x, w, epi):
        load_native(required=True)
        P = sorted_slot.numel()
        N = w.shape[1] // 2 if epi else w.shape[1]
        if out is None:
            out = torch.empty(P, N, dtype=x.dtype, device=x.device)
        nslots = x.shape[0] * k if epi else P
        _call("moe_gemm", out, x, w, sorted_slot, block_expert, k, nslots, epi, BM)
        return out
    return moe_gemm_ref(x, w, sorted_slot, block_expert, k, epi, BM, out)


def moe_combine_ref(y: torch.Tensor, inv: torch.Tensor, weights: torch.Tensor) -> torch.Tensor:
    """The definition of ``moe_combine``: ``out[t] = round(sum_j weights[t, j] * float(y[inv[t*k + j]]))``,
    each product rounded to fp32, added in j order, one final rounding to ``y.dtype``.  A slot with
    ``inv < 0`` contributes nothing."""
    T, k = weights.shape
    rows = inv.reshape(T, k).long()
    acc = torch.zeros(T, y.shape[1], dtype=torch.float32, device=y.device)
    for j in range(k):
        r = rows[:, j]
        term = weights[:, j, None].float() * y[r.clamp_min(0)].float()
        acc = acc + torch.where((r >= 0)[:, None], term, torch.zeros_like(term))
    return acc.to(y.dtype)


def moe_combine(y: torch.Tensor, inv: torch.Tensor, weights: torch.Tensor) -> torch.Tensor:
    """Weighted sum of each token's k expert outputs ``y [P, H]`` (sorted order) -> ``[T, H]``."""
    if (y.is_cuda and y.dtype == torch.bfloat16 and y.is_contiguous() and y.shape[1] % 8 == 0
            and weights.dtype == torch.float32 and weights.shape[1] <= MOE_MAX_TOPK and inv.dtype == torch.int32):
        load_native(required=True)
        out = torch.empty(weights.shape[0], y.shape[1], dtype=y.dtype, device=y.device)
        _call("moe_combine", out, y, inv.contiguous(), weights.contiguous())
        return out
    return moe_combine_ref(y, inv, weights)


def moe_mlp_ref(x: torch.Tensor, router_w: torch.Tensor, gate_up, down, k: int, norm_topk: bool,
                ids: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The definition of ``moe_mlp``, as the per-expert loop: router logits ``x @ router_w^T`` in
    ``x.dtype``, ``moe_route_ref`` (or the forced ``ids`` with the model's own probabilities at them),
    then for every expert its tokens through ``silu(gate) * up`` (fp32, rounded to ``x.dtype``) and
    ``down`` (fp32 accumulate, rounded), combined by ``moe_combine_ref``.  ``gate_up`` and ``down``
    may both be ``Fp8ExpertWeight``: each expert is then dequantised to fp32 first."""
    _expert_pair_quantised(gate_up, down)
    T, H = x.shape
    logits = torch.nn.functional.linear(x, router_w)
    if ids is None:
        ids, weights = moe_route_ref(logits, k, norm_topk)
    else:
        ids = ids.to(torch.int32)
        weights = _route_weights(logits, ids, norm_topk)
    flat = ids.reshape(-1).long()
    y = torch.zeros(T * k, H, dtype=x.dtype, device=x.device)
    for e in torch.unique(flat).tolist():
        slots = torch.nonzero(flat == e).flatten()
        a = x[slots // k].float()
        act = _silu_mul_f32(a @ _expert_f32(gate_up, e).t()).to(x.dtype)
        y[slots] = (act.float() @ _expert_f32(down, e).t()).to(x.dtype)
    inv = torch.arange(T * k, dtype=torch.int32, device=x.device)
    return moe_combine_ref(y, inv, weights)


def moe_mlp_ok(x: torch.Tensor, router_w: torch.Tensor, gate_up, down, k: int) -> bool:
    """Whether the HIP kernels take this MoE block (else ``moe_mlp`` is ``moe_mlp_ref``)."""
    E, I2, H = gate_up.shape
    if _expert_pair_quantised(gate_up, down):
        return (x.is_cuda and x.dim() == 2 and x.shape[0] > 0 and x.dtype == torch.bfloat16
                and gate_up.q.is_cuda and down.q.is_cuda and H % 256 == 0 and (I2 // 2) % 256 == 0
                and gate_up.q.data_ptr() % 16 == 0 and gate_up.scale.data_ptr() % 16 == 0
                and down.q.data_ptr() % 16 == 0 and down.scale.data_ptr() % 16 == 0
                and E <= MOE_MAX_EXPERTS and 1 <= k <= min(E, MOE_MAX_TOPK) and x.shape[0] * k < (1 << 30))
    return (x.is_cuda and x.dim() == 2 and x.shape[0] > 0 and x.dtype == torch.bfloat16
            and gate_up.dtype == torch.bfloat16 and down.dtype == torch.bfloat16
            and gate_up.is_contiguous() and down.is_contiguous() and H % 256 == 0 and (I2 // 2) % 256 == 0
            and E <= MOE_MAX_EXPERTS and 1 <= k <= min(E, MOE_MAX_TOPK) and x.shape[0] * k < (1 << 30))


def moe_mlp(x: torch.Tensor, router_w: torch.Tensor, gate_up, down, k: int, norm_topk: bool,
            ids: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Top-k routed SwiGLU experts (no shared expert): ``x [T, H]``, ``router_w [E, H]``,
    ``gate_up [E, 2I, H]`` (``[gate; up]`` per expert), ``down [E, H, I]`` -> ``[T, H]``.  On the
    GPU: the router through ``linear``, then ``moe_route`` -> ``moe_align`` -> ``moe_gemm`` (SwiGLU)
    -> ``moe_gemm`` (plain) -> ``moe_combine``; nothing is read back, so the block captures into a
    graph.  ``ids`` forces the routing (tests): the weights are then the model's own softmax
    probabilities at those ids.  FP8 weight-only experts: ``gate_up`` and ``down`` both as
    ``Fp8ExpertWeight`` (a mix raises); the two GEMMs are then ``moe_gemm_w8``, nothing else changes."""
    if not moe_mlp_ok(x, router_w, gate_up, down, k):
        return moe_mlp_ref(x, router_w, gate_up, down, k, norm_topk, ids)
    T = x.shape[0]
    E = gate_up.shape[0]
    logits = linear(x, router_w)
    if ids is None:
        ids, weights = moe_route(logits, k, norm_topk)
    else:
        ids = ids.to(device=x.device, dtype=torch.int32).contiguous()
        weights = _route_weights(logits, ids, norm_topk)
    BM = moe_block_rows(T, k, E)
    _counts, _offsets, sorted_slot, block_expert, inv = moe_align(ids, E, BM)
    act = moe_gemm(x, gate_up, sorted_slot, block_expert, k, MOE_EPI_SWIGLU, BM)
    y = moe_gemm(act, down, sorted_slot, block_expert, k, MOE_EPI_PLAIN, BM)
    return moe_combine(y, inv, weights)


# ----------------------------------------------------------------------------
# KV block movement
# ----------------------------------------------------------------------------

def _as16(t: torch.Tensor) -> torch.Tensor:
    """The page-movement kernels copy 16-byte chunks of 16-bit elements: an fp8 cache or buffer
    goes through them as bf16-typed bit patterns of half the head dim (a view, no copy)."""
    return t.view(torch.bfloat16) if t.dtype == KV_FP8 else t


def kv_gather(cache: torch.Tensor, ids: torch.Tensor, out: Optional[torch.Tensor] = None,
              block_major: bool = False) -> torch.Tensor:
    """cache [L,2,NB,...] -> [L,2,n,...] pages of ``ids`` (``block_major``: [n,L,2,...], every
    layer of one page contiguous — the host KV tier's slot layout)."""
    if _native(cache):
        if out is None:
            shape = ((ids.numel(), cache.shape[0], cache.shape[1]) if block_major else
                     (cache.shape[0], cache.shape[1], ids.numel())) + tuple(cache.shape[3:])
            out = torch.empty(shape, dtype=cache.dtype, device=cache.device)
        _call("kv_gather", _as16(out), _as16(cache), ids, bool(block_major))
        return out
    r = cache[:, :, ids.long()]
    if block_major:
        r = r.permute(2, 0, 1, 3, 4, 5).contiguous()
    if out is not None:
        out.copy_(r.view(out.shape))
        return out
    return r


def kv_scatter(cache: torch.Tensor, ids: torch.Tensor, buf: torch.Tensor, block_major: bool = False) -> None:
    if _native(cache):
        _call("kv_scatter", _as16(cache), ids, _as16(buf), bool(block_major))
    elif block_major:
        cache[:, :, ids.long()] = buf.reshape(ids.numel(), cache.shape[0], cache.shape[1],
                                              *cache.shape[3:]).permute(1, 2, 0, 3, 4, 5)
    else:
        cache[:, :, ids.long()] = buf.view(cache.shape[0], cache.shape[1], ids.numel(), *cache.shape[3:])


def kv_copy(cache: torch.Tensor, src: torch.Tensor, dst: torch.Tensor) -> None:
    """Copy pages src[i] -> dst[i] for every layer (src/dst sets must be disjoint)."""
    if _native(cache):
        _call("kv_copy", _as16(cache), src, dst)
    else:
        cache[:, :, dst.long()] = cache[:, :, src.long()]


# ----------------------------------------------------------------------------
# EAGLE tree
# ----------------------------------------------------------------------------

def tree_mask_ref(parent: torch.Tensor):
    B, N = parent.shape
    anc = torch.zeros(B, 64, dtype=torch.long)
    depth = torch.zeros(B, N, dtype=torch.int32)
    par = parent.cpu().tolist()
    for b in range(B):
        for n in range(N):
            m = 1 << n
            d = 0
            p = par[b][n]
            while p >= 0:
                m |= 1 << p
                p = par[b][p]
                d += 1
            if m >= 1 << 63:
                m -= 1 << 64
            anc[b, n] = m
            depth[b, n] = d
    return anc.to(parent.device), depth.to(parent.device)


def tree_mask(parent: torch.Tensor):
    """Ancestor-or-self bitmask [B,64] (int64 bit patterns) and depth [B,N]."""
    if _native(parent):
        B, N = parent.shape
        anc = torch.zeros(B, 64, dtype=torch.long, device=parent.device)
        depth = torch.empty(B, N, dtype=torch.int32, device=parent.device)
        _call("tree_mask", anc, depth, parent)
        return anc, depth
    return tree_mask_ref(parent)


def tree_verify_ref(parent, draft, target, anc, depth, max_path: int):
    B, N = parent.shape
    acc = torch.zeros(B, dtype=torch.int32)
    path = torch.zeros(B, max_path, dtype=torch.int32)
    toks = torch.zeros(B, max_path + 1, dtype=torch.long)
    par, dr, tg = parent.cpu().tolist(), draft.cpu().tolist(), target.cpu().tolist()
    dp = depth.cpu().tolist()
    for b in range(B):
        ok = [False] * N
        for n in range(N):
            if n == 0:
                ok[n] = True
            else:
                ok[n] = ok[par[b][n]] and dr[b][n] == tg[b][par[b][n]]
        best, bd = 0, 0
        for n in range(N):
            if ok[n] and dp[b][n] > bd:
                best, bd = n, dp[b][n]
        acc[b] = bd
        node = best
        for k in range(bd, -1, -1):
            if k < max_path:
                path[b, k] = node
                if k > 0:
                    toks[b, k - 1] = dr[b][node]
            node = par[b][node] if node > 0 else 0
        if bd < max_path + 1:
            toks[b, bd] = tg[b][best]
    dev = parent.device
    return acc.to(dev), path.to(dev), toks.to(dev)


def tree_verify(parent, draft, target, anc, depth, max_path: int):
    """Greedy tree acceptance: (accept_len[B], path[B,max_path], tokens[B,max_path+1])."""
    if _native(parent):
        B = parent.shape[0]
        acc = torch.empty(B, dtype=torch.int32, device=parent.device)
        path = torch.zeros(B, max_path, dtype=torch.int32, device=parent.device)
        toks = torch.zeros(B, max_path + 1, dtype=torch.long, device=parent.device)
        _call("tree_verify", acc, path, toks, parent, draft, target, anc, depth)
        return acc, path, toks
    return tree_verify_ref(parent, draft, target, anc, depth, max_path)
