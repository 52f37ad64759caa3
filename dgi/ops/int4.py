"""INT4 weight-only quantisation (W4A16) with per-group scales and zero points — the AWQ family:
the weight container, a round-to-nearest quantiser and the repacker of AWQ checkpoints.

    w[n, k] = (code[n, k] - zero[n, k // 128]) * scale[n, k // 128]

``code`` and ``zero`` are integers in 0..15, ``scale`` is a finite fp16, the group is 128 elements
of a row.  Activations, accumulation and outputs stay as they are.  ``dgi.ops.linear`` takes an
``Int4Weight`` wherever it takes a weight tensor.

The experts of a MoE layer are held the same way, stacked: ``Int4ExpertWeight``, which
``dgi.ops.moe_gemm`` / ``moe_mlp`` take wherever they take an ``[E, N, K]`` tensor.
"""
from __future__ import annotations

from typing import Optional

import torch

INT4_GROUP = 128
_SLAB = 16 << 20            # elements of an int64 temporary: packing and unpacking work in row slabs
_NIBBLE_OF = (0, 4, 1, 5, 2, 6, 3, 7)      # element j of a dword sits in nibble (j >> 1) + 4 (j & 1)
_ZERO_BIAS = 0x4300         # the bf16 bits of 128.0: 0x4300 + zero is 128 + zero as a bf16
# AWQ "GEMM" packing: nibble i of an int32 holds output column 8c + AWQ_ORDER[i].  Written down from
# memory of AutoAWQ's packer (order_map) and its reverse in the unpackers; no AWQ package was at hand
# to check it against, and the AWQ integration of the transformers package this was written beside
# delegates packing to an external kernel package and does not spell the order out.
AWQ_ORDER = (0, 2, 4, 6, 1, 3, 5, 7)


def _to_i32(d: torch.Tensor) -> torch.Tensor:
    """An int64 tensor of values 0 .. 2^32 - 1 as the int32 of the same 32 bits."""
    return torch.where(d >= (1 << 31), d - (1 << 32), d).to(torch.int32)


class Int4Weight:
    """An [N, K] weight in the layout of ``dgi/csrc/skinny_gemm_int4.hip`` — the kernel's own,
    chosen at load time, not AWQ's:

    ``q`` [N, K/8] int32.  Group ``h`` of a row (128 elements) is dwords ``16h .. 16h + 15``; dword
      ``16h + 4g + c`` (``g``, ``c`` in 0..3) holds ``k = 128h + 32c + 8g + j`` for ``j`` in 0..7, element
      ``j`` in nibble ``(j >> 1) + 4 (j & 1)``.  Lane group ``g`` of a wave then finds fragment ``c`` of an
      MFMA over 32 contiguous ``k`` in one dword, and ``(dword >> 4p) & 0x000F000F`` is the pair
      ``j = 2p, 2p + 1`` in the two halves of a register.
    ``sz`` [N, K/128] int32, one per group: the low half is the scale's fp16 bits, the high half
      ``0x4300 + zero`` (``128 + zero`` as a bf16, the form the kernel subtracts).

    ``Int4Weight.pack(code, zero, scale)`` builds one from the plain tensors; ``codes()``, ``zeros()``
    and ``scales()`` give them back."""
    __slots__ = ("q", "sz", "scratch")

    def __init__(self, q: torch.Tensor, sz: torch.Tensor, scratch: Optional[torch.Tensor] = None):
        if q.dtype != torch.int32 or q.dim() != 2 or not q.is_contiguous() or (8 * q.shape[1]) % INT4_GROUP:
            raise ValueError("Int4Weight: q must be a contiguous [N, K/8] int32 tensor with K % 128 == 0")
        if (sz.dtype != torch.int32 or sz.shape != (q.shape[0], 8 * q.shape[1] // INT4_GROUP)
                or not sz.is_contiguous()):
            raise ValueError("Int4Weight: sz must be a contiguous [N, K/128] int32 tensor")
        if sz.device != q.device:
            raise ValueError("Int4Weight: q and sz on one device")
        self.q = q
        self.sz = sz
        # flat bf16 buffer of >= N*K elements the dequantised copy is written to for the shapes
        # the int4 kernel does not take (shared by every layer of a model); None: allocated per call
        self.scratch = scratch

    @classmethod
    def pack(cls, code: torch.Tensor, zero: torch.Tensor, scale: torch.Tensor) -> "Int4Weight":
        """``code`` [N, K] and ``zero`` [N, K/128] integers in 0..15, ``scale`` [N, K/128] fp16."""
        if code.dim() != 2 or code.shape[1] % INT4_GROUP:
            raise ValueError("Int4Weight.pack: code is [N, K] with K % 128 == 0")
        N, K = code.shape
        H = K // INT4_GROUP
        if zero.shape != (N, H) or scale.shape != (N, H) or scale.dtype != torch.float16:
            raise ValueError("Int4Weight.pack: zero and scale are [N, K/128], scale fp16")
        if not bool(torch.isfinite(scale).all()):
            raise ValueError("Int4Weight.pack: scales must be finite")
        for name, t in (("code", code), ("zero", zero)):
            if t.numel() and (int(t.min()) < 0 or int(t.max()) > 15):
                raise ValueError(f"Int4Weight.pack: {name} outside 0..15")
        shifts = torch.tensor([4 * p for p in _NIBBLE_OF], dtype=torch.int64, device=code.device)
        q = torch.empty(N, K // 8, dtype=torch.int32, device=code.device)
        step = max(1, _SLAB // max(1, K))
        for r0 in range(0, N, step):
            c = code[r0:r0 + step].to(torch.int64).view(-1, H, 4, 4, 8).permute(0, 1, 3, 2, 4)    # [n, h, g, c, j]
            q[r0:r0 + step] = _to_i32((c << shifts).sum(-1)).reshape(-1, K // 8)
        sz = (scale.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF) | ((zero.to(torch.int32) + _ZERO_BIAS) << 16)
        return cls(q, sz.contiguous())

    @property
    def shape(self) -> torch.Size:
        return torch.Size((self.q.shape[0], 8 * self.q.shape[1]))

    @property
    def device(self) -> torch.device:
        return self.q.device

    def nbytes(self) -> int:
        return 4 * (self.q.numel() + self.sz.numel())

    def codes(self, r0: int = 0, r1: Optional[int] = None) -> torch.Tensor:
        """[N, K] uint8 codes (of rows ``r0 .. r1``) in the plain order."""
        q = self.q[r0:r1]
        K = self.shape[1]
        shifts = torch.tensor([4 * p for p in _NIBBLE_OF], dtype=torch.int32, device=q.device)
        nib = (q.view(-1, K // INT4_GROUP, 4, 4, 1) >> shifts) & 15            # [n, h, g, c, j]
        return nib.permute(0, 1, 3, 2, 4).reshape(-1, K).to(torch.uint8)

    def zeros(self) -> torch.Tensor:
        return (((self.sz >> 16) & 0xFFFF) - _ZERO_BIAS).to(torch.uint8)

    def scales(self) -> torch.Tensor:
        return (self.sz & 0xFFFF).to(torch.int16).view(torch.float16)

    def dequant(self, dtype: torch.dtype = torch.float32) -> torch.Tensor:
        """The decoded weight: ``float(code - zero) * float(scale)`` in fp32 (exact: a 5-bit integer
        times an fp16), then ``dtype``."""
        N, K = self.shape
        out = torch.empty(N, K, dtype=dtype, device=self.q.device)
        z, s = self.zeros().float(), self.scales().float()
        step = max(1, _SLAB // max(1, K))
        for r0 in range(0, N, step):
            c = self.codes(r0, r0 + step).float().view(-1, K // INT4_GROUP, INT4_GROUP)
            out[r0:r0 + step] = ((c - z[r0:r0 + step, :, None]) * s[r0:r0 + step, :, None]).view(-1, K).to(dtype)
        return out

    def __repr__(self) -> str:
        return f"Int4Weight(shape={tuple(self.shape)}, device={self.q.device})"


def quantize_int4(w: torch.Tensor) -> Int4Weight:
    """Asymmetric round-to-nearest per 128-group of K.  With ``lo = min(group, 0)`` and
    ``hi = max(group, 0)``: ``scale = fp16((hi - lo) / 15 * (1 + 2^-10))`` — rounded up, so that 15 steps
    cover the range whichever way fp16 rounds — and at least 2^-14 (the smallest normal fp16);
    ``zero = round(-lo / scale)``, ``code = clamp(round(w / scale) + zero, 0, 15)``.  The range holds 0,
    so the zero point is a code and nothing saturates: the error is at most half a step."""
    if w.dim() != 2 or w.shape[1] % INT4_GROUP:
        raise ValueError("quantize_int4: a [N, K] weight with K % 128 == 0")
    N, K = w.shape
    H = K // INT4_GROUP
    code = torch.empty(N, K, dtype=torch.uint8, device=w.device)
    zero = torch.empty(N, H, dtype=torch.uint8, device=w.device)
    scale = torch.empty(N, H, dtype=torch.float16, device=w.device)
    step = max(1, _SLAB // max(1, K))      # bounded fp32 temporaries
    with torch.no_grad():
        for r0 in range(0, N, step):
            wf = w[r0:r0 + step].float().view(-1, H, INT4_GROUP)
            lo = wf.amin(dim=2).clamp_(max=0.0)
            hi = wf.amax(dim=2).clamp_(min=0.0)
            s16 = ((hi - lo) / 15.0 * (1.0 + 2.0 ** -10)).clamp_(min=2.0 ** -14).to(torch.float16)
            s = s16.float()
            z = torch.round(-lo / s).clamp_(0, 15)
            c = (torch.round(wf / s[:, :, None]) + z[:, :, None]).clamp_(0, 15)
            code[r0:r0 + step] = c.view(-1, K).to(torch.uint8)
            zero[r0:r0 + step] = z.to(torch.uint8)
            scale[r0:r0 + step] = s16
    return Int4Weight.pack(code, zero, scale)


class Int4ExpertWeight:
    """The experts of a MoE layer, INT4 weight-only: ``Int4Weight``'s row layout stacked over experts,
    ``q`` [E, N, K/8] int32 and ``sz`` [E, N, K/128] int32 (rows are independent, so ``[gate; up]`` and
    the expert index are row offsets).  ``dgi.ops.moe_gemm`` / ``moe_mlp`` take it wherever they take
    an ``[E, N, K]`` tensor."""
    __slots__ = ("q", "sz")

    def __init__(self, q: torch.Tensor, sz: torch.Tensor):
        if q.dtype != torch.int32 or q.dim() != 3 or not q.is_contiguous() or (8 * q.shape[2]) % INT4_GROUP:
            raise ValueError("Int4ExpertWeight: q must be a contiguous [E, N, K/8] int32 tensor with K % 128 == 0")
        if (sz.dtype != torch.int32 or sz.shape != (q.shape[0], q.shape[1], 8 * q.shape[2] // INT4_GROUP)
                or not sz.is_contiguous()):
            raise ValueError("Int4ExpertWeight: sz must be a contiguous [E, N, K/128] int32 tensor")
        if sz.device != q.device:
            raise ValueError("Int4ExpertWeight: q and sz must be on one device")
        self.q = q
        self.sz = sz

    @property
    def shape(self) -> torch.Size:
        return torch.Size((self.q.shape[0], self.q.shape[1], 8 * self.q.shape[2]))

    @property
    def device(self) -> torch.device:
        return self.q.device

    def nbytes(self) -> int:
        return 4 * (self.q.numel() + self.sz.numel())

    def __getitem__(self, e: int) -> Int4Weight:
        """Expert ``e`` as a dense ``Int4Weight`` (views of the codes and scale words, nothing copied)."""
        return Int4Weight(self.q[e], self.sz[e])

    def dequant(self, dtype: torch.dtype = torch.float32) -> torch.Tensor:
        """``(code - zero) * scale`` in fp32, rounded once to ``dtype``: ``[E, N, K]``, one expert at a time."""
        out = torch.empty(tuple(self.shape), dtype=dtype, device=self.q.device)
        for e in range(self.q.shape[0]):
            out[e] = self[e].dequant(dtype)
        return out

    def __repr__(self) -> str:
        return f"Int4ExpertWeight(shape={tuple(self.shape)}, device={self.q.device})"


def quantize_int4_experts(w: torch.Tensor) -> Int4ExpertWeight:
    """``quantize_int4`` of every expert of ``w [E, N, K]``, written into one ``Int4ExpertWeight``:
    bit-identical words to ``quantize_int4(w[e])``, one expert at a time (the temporaries are those of
    one expert's quantiser)."""
    if w.dim() != 3 or w.shape[2] % INT4_GROUP:
        raise ValueError("quantize_int4_experts: an [E, N, K] weight with K % 128 == 0")
    E, N, K = w.shape
    q = torch.empty(E, N, K // 8, dtype=torch.int32, device=w.device)
    sz = torch.empty(E, N, K // INT4_GROUP, dtype=torch.int32, device=w.device)
    for e in range(E):
        one = quantize_int4(w[e])
        q[e].copy_(one.q)
        sz[e].copy_(one.sz)
        del one
    return Int4ExpertWeight(q, sz)


def _awq_unpack(packed: torch.Tensor) -> torch.Tensor:
    """[R, C] int32 of eight nibbles -> [R, 8C] uint8 in column order."""
    shifts = torch.tensor([4 * AWQ_ORDER.index(j) for j in range(8)], dtype=torch.int32, device=packed.device)
    return ((packed[:, :, None] >> shifts) & 15).reshape(packed.shape[0], -1).to(torch.uint8)


def int4_from_awq(qweight: torch.Tensor, qzeros: torch.Tensor, scales: torch.Tensor) -> Int4Weight:
    """Repack AWQ "GEMM"-version tensors of one linear layer (in_features K, out_features N,
    group size 128): ``qweight`` [K, N/8] int32, ``qzeros`` [K/128, N/8] int32, ``scales`` [K/128, N]
    fp16, with ``w[k, n] = (code[k, n] - zero[k // 128, n]) * scale[k // 128, n]``.  Eight 4-bit values
    share an int32 along N; nibble ``i`` holds column ``8c + AWQ_ORDER[i]``.

    The nibble order is written as remembered from AutoAWQ (see ``AWQ_ORDER``); it could not be
    checked against an AWQ package or a published checkpoint when this was written."""
    if qweight.dtype != torch.int32 or qzeros.dtype != torch.int32 or qweight.dim() != 2 or qzeros.dim() != 2:
        raise ValueError("int4_from_awq: qweight and qzeros are 2-D int32 tensors")
    K, N = qweight.shape[0], 8 * qweight.shape[1]
    if K % INT4_GROUP or qzeros.shape != (K // INT4_GROUP, N // 8) or scales.shape != (K // INT4_GROUP, N):
        raise ValueError(f"int4_from_awq: qweight [K, N/8] with K % 128 == 0, qzeros [K/128, N/8], scales [K/128, N]; "
                         f"got {tuple(qweight.shape)}, {tuple(qzeros.shape)}, {tuple(scales.shape)}")
    if scales.dtype != torch.float16:
        raise ValueError("int4_from_awq: scales must be fp16")
    return Int4Weight.pack(_awq_unpack(qweight).t().contiguous(), _awq_unpack(qzeros).t().contiguous(),
                           scales.t().contiguous())


def int4_cat(parts) -> Int4Weight:
    """Concatenate along N (q|k|v, gate|up): rows are stored independently of each other."""
    return Int4Weight(torch.cat([p.q for p in parts], 0), torch.cat([p.sz for p in parts], 0))
