"""FP8 weight-only quantisation (W8A16): the weight container and its quantiser.

A projection is held as OCP e4m3 codes (``torch.float8_e4m3fn``, not the ``fnuz``
variant of earlier hardware) with one fp32 scale per output channel; activations,
accumulation and outputs stay as they are.  ``dgi.ops.linear`` takes an ``Fp8Weight``
wherever it takes a weight tensor.

The experts of a MoE layer are held the same way, stacked: ``Fp8ExpertWeight`` (codes
``[E, N, K]``, scales ``[E, N]``), which ``dgi.ops.moe_gemm`` / ``moe_mlp`` take wherever they
take an ``[E, N, K]`` tensor.
"""
from __future__ import annotations

from typing import Optional

import torch

E4M3_MAX = 448.0


class Fp8Weight:
    """``q`` [N, K] e4m3 codes, ``scale`` [N] fp32: the weight is ``q * scale[:, None]``."""
    __slots__ = ("q", "scale", "scratch", "act")

    def __init__(self, q: torch.Tensor, scale: torch.Tensor, scratch: Optional[torch.Tensor] = None,
                 act: Optional[str] = None):
        if q.dtype != torch.float8_e4m3fn or q.dim() != 2 or not q.is_contiguous():
            raise ValueError("Fp8Weight: q must be a contiguous [N, K] float8_e4m3fn tensor")
        if scale.dtype != torch.float32 or scale.shape != (q.shape[0],) or not scale.is_contiguous():
            raise ValueError("Fp8Weight: scale must be a contiguous [N] float32 tensor")
        self.q = q
        self.scale = scale
        # flat bf16 buffer of >= N*K elements the dequantised copy is written to for the shapes
        # the fp8 kernel does not take (shared by every layer of a model); None: allocated per call
        self.scratch = scratch
        if act not in (None, "fp8"):
            raise ValueError("Fp8Weight: act must be None or 'fp8'")
        # "fp8": W8A8 — steps of at least ops.W8A8_MIN_M rows quantise their activations per
        # token to e4m3 and run the e4m3 GEMM; None: W8A16 at every row count
        self.act = act

    @property
    def shape(self) -> torch.Size:
        return self.q.shape

    @property
    def device(self) -> torch.device:
        return self.q.device

    def nbytes(self) -> int:
        return self.q.numel() + 4 * self.scale.numel()

    def dequant(self, dtype: torch.dtype = torch.float32) -> torch.Tensor:
        """``q * scale`` in fp32, rounded once to ``dtype``."""
        return (self.q.float() * self.scale[:, None]).to(dtype)

    def __repr__(self) -> str:
        return f"Fp8Weight(shape={tuple(self.q.shape)}, device={self.q.device})"


class Fp8ExpertWeight:
    """The experts of a MoE layer, FP8 weight-only: ``q`` [E, N, K] e4m3 codes, ``scale`` [E, N]
    fp32 (one per expert and output channel); expert e's weight is ``q[e] * scale[e][:, None]``.
    ``dgi.ops.moe_gemm`` / ``moe_mlp`` take it wherever they take an ``[E, N, K]`` tensor."""
    __slots__ = ("q", "scale")

    def __init__(self, q: torch.Tensor, scale: torch.Tensor):
        if q.dtype != torch.float8_e4m3fn or q.dim() != 3 or not q.is_contiguous():
            raise ValueError("Fp8ExpertWeight: q must be a contiguous [E, N, K] float8_e4m3fn tensor")
        if scale.dtype != torch.float32 or scale.shape != q.shape[:2] or not scale.is_contiguous():
            raise ValueError("Fp8ExpertWeight: scale must be a contiguous [E, N] float32 tensor")
        if scale.device != q.device:
            raise ValueError("Fp8ExpertWeight: q and scale must be on one device")
        self.q = q
        self.scale = scale

    @property
    def shape(self) -> torch.Size:
        return self.q.shape

    @property
    def device(self) -> torch.device:
        return self.q.device

    def nbytes(self) -> int:
        return self.q.numel() + 4 * self.scale.numel()

    def __getitem__(self, e: int) -> Fp8Weight:
        """Expert ``e`` as a dense ``Fp8Weight`` (views of the codes and scales, nothing copied)."""
        return Fp8Weight(self.q[e], self.scale[e])

    def dequant(self, dtype: torch.dtype = torch.float32) -> torch.Tensor:
        """``q * scale`` in fp32, rounded once to ``dtype``: ``[E, N, K]``, one expert at a time."""
        out = torch.empty(self.q.shape, dtype=dtype, device=self.q.device)
        for e in range(self.q.shape[0]):
            out[e] = self[e].dequant(dtype)
        return out

    def __repr__(self) -> str:
        return f"Fp8ExpertWeight(shape={tuple(self.q.shape)}, device={self.q.device})"


def quantize_fp8_experts(w: torch.Tensor) -> Fp8ExpertWeight:
    """``quantize_fp8`` of every expert of ``w [E, N, K]``, written into one ``Fp8ExpertWeight``:
    bit-identical codes and scales to ``quantize_fp8(w[e])``, one expert at a time (the fp32
    temporaries are those of one expert's quantiser)."""
    if w.dim() != 3:
        raise ValueError("quantize_fp8_experts: an [E, N, K] weight")
    E, N, K = w.shape
    q = torch.empty(E, N, K, dtype=torch.float8_e4m3fn, device=w.device)
    scale = torch.empty(E, N, dtype=torch.float32, device=w.device)
    for e in range(E):
        one = quantize_fp8(w[e])
        q[e].copy_(one.q)
        scale[e].copy_(one.scale)
        del one
    return Fp8ExpertWeight(q, scale)


def quantize_fp8(w: torch.Tensor) -> Fp8Weight:
    """Per-output-channel symmetric e4m3: ``scale[n] = max|w[n]| / 448`` (1 for a zero row).

    The quotient is clamped before the cast: torch's cast does not saturate (470 becomes NaN)."""
    if w.dim() != 2:
        raise ValueError("quantize_fp8: a [N, K] weight")
    N, K = w.shape
    q = torch.empty(N, K, dtype=torch.float8_e4m3fn, device=w.device)
    scale = torch.empty(N, dtype=torch.float32, device=w.device)
    step = max(1, (256 << 20) // (4 * max(1, K)))      # bounded fp32 temporaries
    with torch.no_grad():
        for r0 in range(0, N, step):
            wf = w[r0:r0 + step].float()
            amax = wf.abs().amax(dim=1)
            s = torch.where(amax > 0, amax / E4M3_MAX, torch.ones_like(amax))
            scale[r0:r0 + step] = s
            q[r0:r0 + step] = (wf / s[:, None]).clamp_(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)
    return Fp8Weight(q, scale)
