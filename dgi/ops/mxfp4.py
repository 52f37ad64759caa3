"""MXFP4 weight-only quantisation (W4A16): the weight container and its quantiser.

OCP Microscaling FP4: a projection is held as e2m1 codes, two per byte, with one e8m0
scale per 32 elements of a row; activations, accumulation and outputs stay as they are.
``dgi.ops.linear`` takes an ``Mxfp4Weight`` wherever it takes a weight tensor.

A nibble is ``s e e m``: the magnitudes by code 0..7 are 0, 0.5, 1, 1.5, 2, 3, 4, 6.  A scale
code ``e`` means ``2^(e - 127)``.  The format is specified here for scale codes 2..252, where
every decoded weight is a normal bf16 number and ``e << 23`` is the scale as an fp32 bit
pattern; codes outside that range need not decode correctly.
"""
from __future__ import annotations

from typing import Optional

import torch

MXFP4_BLOCK = 32
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
E8M0_MIN, E8M0_MAX = 2, 252
_ROW_BUDGET = 64 << 20      # elements of a temporary: the quantiser and dequant() work in row slabs


def _table(device, dtype=torch.float32) -> torch.Tensor:
    return torch.tensor(E2M1_VALUES + tuple(-v for v in E2M1_VALUES), dtype=dtype, device=device)


class Mxfp4Weight:
    """``q`` [N, K/2] uint8 (element 2j in the low nibble of byte j, 2j+1 in the high nibble),
    ``scale`` [N, K/32] uint8 e8m0: the weight is ``elem[n, k] * 2^(scale[n, k // 32] - 127)``."""
    __slots__ = ("q", "scale", "scratch")

    def __init__(self, q: torch.Tensor, scale: torch.Tensor, scratch: Optional[torch.Tensor] = None):
        if q.dtype != torch.uint8 or q.dim() != 2 or not q.is_contiguous() or (2 * q.shape[1]) % MXFP4_BLOCK:
            raise ValueError("Mxfp4Weight: q must be a contiguous [N, K/2] uint8 tensor with K % 32 == 0")
        if (scale.dtype != torch.uint8 or scale.shape != (q.shape[0], 2 * q.shape[1] // MXFP4_BLOCK)
                or not scale.is_contiguous()):
            raise ValueError("Mxfp4Weight: scale must be a contiguous [N, K/32] uint8 (e8m0) tensor")
        if scale.device != q.device:
            raise ValueError("Mxfp4Weight: q and scale on one device")
        self.q = q
        self.scale = scale
        # flat bf16 buffer of >= N*K elements the dequantised copy is written to for the shapes
        # the mxfp4 kernel does not take (shared by every layer of a model); None: allocated per call
        self.scratch = scratch

    @property
    def shape(self) -> torch.Size:
        return torch.Size((self.q.shape[0], 2 * self.q.shape[1]))

    @property
    def device(self) -> torch.device:
        return self.q.device

    def nbytes(self) -> int:
        return self.q.numel() + self.scale.numel()

    def dequant(self, dtype: torch.dtype = torch.float32) -> torch.Tensor:
        """The decoded weight: a 16-entry table lookup times ``2^(scale - 127)`` in fp32 (exact),
        then ``dtype`` (exact in bf16 for scale codes 2..252)."""
        N, K = self.shape
        out = torch.empty(N, K, dtype=dtype, device=self.q.device)
        table = _table(self.q.device)
        step = max(1, _ROW_BUDGET // max(1, K))
        for r0 in range(0, N, step):
            q = self.q[r0:r0 + step]
            codes = torch.stack((q & 0xF, q >> 4), dim=-1).view(q.shape[0], K)
            s = (self.scale[r0:r0 + step].to(torch.int32) << 23).view(torch.float32)
            vals = table[codes.to(torch.int32)].view(q.shape[0], K // MXFP4_BLOCK, MXFP4_BLOCK) * s[:, :, None]
            out[r0:r0 + step] = vals.view(q.shape[0], K).to(dtype)
        return out

    def __repr__(self) -> str:
        return f"Mxfp4Weight(shape={tuple(self.shape)}, device={self.q.device})"


def quantize_mxfp4(w: torch.Tensor) -> Mxfp4Weight:
    """Per 32-block of K: with ``amax = f * 2^x``, ``f`` in [0.5, 1) (``frexp``), the block exponent is
    ``x - 3`` if ``f <= 0.75`` else ``x - 2`` — the smallest ``E`` with ``amax <= 6 * 2^E``, so nothing
    saturates — and the scale code ``clamp(E + 127, 2, 252)`` (127 for a zero block).  Elements round
    to the nearest e2m1 grid point, ties to the code with mantissa bit 0; the sign bit is kept.

    Integer and comparison arithmetic only (no floating ``log2``), so a bf16 and an fp32 tensor of the
    same values give the same codes on every device."""
    if w.dim() != 2 or w.shape[1] % MXFP4_BLOCK:
        raise ValueError("quantize_mxfp4: a [N, K] weight with K % 32 == 0")
    N, K = w.shape
    nb = K // MXFP4_BLOCK
    q = torch.empty(N, K // 2, dtype=torch.uint8, device=w.device)
    scale = torch.empty(N, nb, dtype=torch.uint8, device=w.device)
    step = max(1, _ROW_BUDGET // max(1, K))      # bounded fp32 temporaries
    with torch.no_grad():
        for r0 in range(0, N, step):
            wf = w[r0:r0 + step].float().view(-1, nb, MXFP4_BLOCK)
            amax = wf.abs().amax(dim=2)
            f, x = torch.frexp(amax)
            e = torch.where(f <= 0.75, x - 3, x - 2).to(torch.int32)
            code = torch.where(amax > 0, (e + 127).clamp_(E8M0_MIN, E8M0_MAX), torch.full_like(e, 127))
            scale[r0:r0 + step] = code.to(torch.uint8)
            # |w| * 2^-E, the multiplier built from its bits (254 - code is in 2..252: a normal number)
            inv = ((254 - code) << 23).view(torch.float32)
            v = wf.abs() * inv[:, :, None]
            # midpoints of the grid; a tie goes to the neighbour whose mantissa bit is 0
            c = ((v > 0.25).to(torch.uint8) + (v >= 0.75).to(torch.uint8) + (v > 1.25).to(torch.uint8)
                 + (v >= 1.75).to(torch.uint8) + (v > 2.5).to(torch.uint8) + (v >= 3.5).to(torch.uint8)
                 + (v > 5.0).to(torch.uint8))
            c |= torch.signbit(wf).to(torch.uint8) << 3
            c = c.view(-1, K // 2, 2)
            q[r0:r0 + step] = c[:, :, 0] | (c[:, :, 1] << 4)
    return Mxfp4Weight(q, scale)
