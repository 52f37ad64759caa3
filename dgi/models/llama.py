"""Native Llama-family decoder for the MI355X runtime (Llama-3 8B / 70B, Qwen2 / Qwen2.5, GLM-4).

Replaces the HF modules the reference executes (worker/engines/llm.py:22-69,
worker/distributed/model_shard.py:28-246).  Per layer the step runs

    fused_add_rmsnorm (HIP) -> QKV GEMM (hipBLASLt) -> RoPE + paged KV write (HIP)
    -> paged decode / prefill attention (HIP, MFMA) -> O GEMM
    -> fused_add_rmsnorm (HIP) -> gate|up GEMM -> SiLU*mul (HIP) -> down GEMM

with fused QKV and gate|up weights so each layer issues 4 GEMMs.  Qwen2's biased
q/k/v projections ride in the QKV GEMM's bias epilogue (hipBLASLt), so the
family adds no kernel; GLM-4 adds biased QKV and half-dim interleaved RoPE
(``rope_cache`` mode 1 over the first ``rotary_dim`` dims); Qwen3 drops the bias and
normalises every q and k head before RoPE, inside the writer (``qknorm_rope_cache``); Qwen3-MoE
replaces every layer's MLP by a top-k routed set of SwiGLU experts (``ops.moe_mlp``).  A model
object may hold any contiguous layer range (pipeline stage): stage 0 owns the
embedding, the last stage the final norm and LM head, exactly like the
reference's ``ModelShard`` (model_shard.py:28-59).  Between stages a single
hidden tensor travels: the residual stream (h + residual) — the next stage
re-normalises it, which is bit-identical to the fused add it replaces.
"""
from __future__ import annotations

import contextlib
import math
import os
from typing import Optional

import torch
import torch.nn.functional as F

from dgi import ops
from dgi.models.config import ModelConfig
from dgi.runtime.batch import AttnMeta



# DGI_TRIM_LAST_LAYER=0 runs the last layer's o-proj and MLP on every row (A/B switch)
TRIM_LAST_LAYER = os.environ.get("DGI_TRIM_LAST_LAYER", "1") != "0"
# mixed steps: decode-row attention on a side stream beside the prefill-row attention
ATTN_OVERLAP = os.environ.get("DGI_ATTN_OVERLAP", "1") == "1"
# steps of <= 16 rows that carry prefill tokens (an EAGLE tree verify: N tree nodes per sequence
# under a tree mask) take the fused decode layers too — the qkv / gate_up kernels are per-row
# (norm prologue, RoPE + paged-KV epilogue at each row's own position / slot) and the attention
# dispatch already splits decode and prefill rows; 5 kernels per layer instead of 9
FUSED_SMALL_PREFILL = os.environ.get("DGI_FUSED_SMALL_PREFILL", "1") == "1"
# Fused-norm layers (``LlamaModel._forward_layers_folded``): the RMSNorm gains are folded into the
# qkv / gate_up weights once (``fold_norms``), the o-proj and down GEMMs add into the residual
# stream in their epilogue and emit its per-row sums of squares, and the qkv / gate_up GEMMs
# scale their rows by the resulting rstd — no norm kernel and no normalised copy of the stream
# between the four projections (dgi/csrc/mfma_gemm.hip EPI 2-5).  "1" (default): every eligible
# step of >= NORM_FOLD_MIN_ROWS rows of a model the engine routes GEMMs for (a shipped or measured
# routing table: the production shapes) — measured faster on the 512-row decode-role step (77.6 vs
# 78.5 ms) and on the headline's mixed steps (profiles/r6_norm/); "force": every eligible step of
# any model; "table": only where the routing table (timed on one warm weight) prices the all-MFMA
# layer at least as fast as the best mix plus the norm kernels; "0": off.  Smaller steps keep the
# skinny / fused-decode kernels.  (The fused layers round differently from the unfused ones — no
# normalised bf16 copy of the stream — so a model whose steps switch between the two computes
# near-tied greedy tokens batch-dependently; test-size engines without a routing table stay unfused.)
NORM_FOLD = os.environ.get("DGI_NORM_FOLD", "1")
NORM_FOLD_MIN_ROWS = int(os.environ.get("DGI_NORM_FOLD_MIN_ROWS", "256"))
# fused-norm layers: RoPE + the paged-KV write in the qkv GEMM's epilogue (EPI 5) where the geometry
# allows (NeoX rotary over 128-dim heads, q / kv column blocks of 256); "0" keeps rope_cache
NORM_FOLD_ROPE = os.environ.get("DGI_NORM_FOLD_ROPE", "1") != "0"


def fold_decision(mode: str, rows: int, fold_impl) -> bool:
    """Whether a GPU step of ``rows`` rows runs the fused-norm layers under ``DGI_NORM_FOLD`` =
    ``mode`` (shape eligibility aside): ``fold_impl`` is the model's routing-table rule (None when
    the engine routes no GEMMs for it, e.g. test-size models)."""
    if mode == "0" or rows < NORM_FOLD_MIN_ROWS:
        return False
    if mode == "force":
        return True
    if fold_impl is None:
        return False
    return mode == "1" or (mode == "table" and bool(fold_impl(rows)))


def _ss_cols(hidden: int) -> int:
    """Columns of the fused-norm row statistics: one partial per 256-column tile of the stream,
    padded to a multiple of 8 (the consumer's vector loads; the pad columns stay zero)."""
    return (hidden // 256 + 7) // 8 * 8


class LlamaLayerWeights:
    __slots__ = ("in_norm", "qkv", "o", "post_norm", "gate_up", "down", "qkv_bias", "q_norm", "k_norm",
                 "router", "experts_gate_up", "experts_down")

    def __init__(self, in_norm, qkv, o, post_norm, gate_up, down, qkv_bias=None, q_norm=None, k_norm=None,
                 router=None, experts_gate_up=None, experts_down=None):
        self.in_norm, self.qkv, self.o = in_norm, qkv, o
        self.post_norm, self.gate_up, self.down = post_norm, gate_up, down
        self.qkv_bias = qkv_bias   # [qkv_size] for Qwen2, else None (fused into the QKV GEMM epilogue)
        # [head_dim] gains of the per-head q / k RMSNorm for Qwen3, else None (ops.qknorm_rope_cache)
        self.q_norm, self.k_norm = q_norm, k_norm
        # MoE layers (Qwen3-MoE): router [E, H], experts' [gate; up] [E, 2I, H] and down [E, H, I];
        # their gate_up and down are None (ops.moe_mlp)
        self.router, self.experts_gate_up, self.experts_down = router, experts_gate_up, experts_down


QUANT_SLOTS = ("qkv", "o", "gate_up", "down")    # the projections quantize_weights replaces
EXPERT_SLOTS = ("experts_gate_up", "experts_down")    # the tensors quantize_experts replaces


def _rand(shape, gen, device, dtype, std):
    t = torch.empty(shape, device=device, dtype=dtype)
    t.normal_(0.0, std, generator=gen)
    return t


class LlamaModel:
    """Layer range [layer_start, layer_end) of a Llama causal LM."""

    def __init__(self, cfg: ModelConfig, device: torch.device | str = "cpu", dtype=torch.bfloat16,
                 layer_start: int = 0, layer_end: Optional[int] = None, has_embed: Optional[bool] = None,
                 has_head: Optional[bool] = None, seed: int = 0, init: str = "random",
                 checkpoint: Optional[str] = None):
        self.cfg = cfg
        self.device = torch.device(device)
        self.dtype = dtype
        self.layer_start = layer_start
        self.layer_end = cfg.num_layers if layer_end is None else layer_end
        self.has_embed = (layer_start == 0) if has_embed is None else has_embed
        self.has_head = (self.layer_end == cfg.num_layers) if has_head is None else has_head
        self.num_local_layers = self.layer_end - self.layer_start
        self.scale = 1.0 / math.sqrt(cfg.head_dim)
        self.kv_cache: Optional[torch.Tensor] = None  # [L_local, 2, NB, nkv, bs, hd]
        # fp8 KV pool (float8_e4m3fn pages): its per (layer, K/V, kv head) scales and their stored
        # inverses, [L_local, 2, nkv] fp32 each (``bind_kv``); unused with a bf16 pool
        self.kv_scale: Optional[torch.Tensor] = None
        self.kv_inv_scale: Optional[torch.Tensor] = None
        self.layers: list[LlamaLayerWeights] = []
        self.embed = self.norm = self.lm_head = None
        # EAGLE-3 feature taps: global layer ids whose output residual stream is kept
        self.capture_layers: tuple = ()
        self.captured: dict = {}
        self.force_fused = False
        # tensor parallelism: in-place sum of partial outputs across the TP group
        # after the row-parallel O and down projections (dgi.parallel.tensor)
        self.reduce = None
        # MLP row padding (dgi.runtime.gemm_pad): T -> rows to run gate_up/down on
        self.mlp_pad = None
        self.mlp_impl = None     # rows -> (gate_up on the MFMA SwiGLU kernel, down on the MFMA kernel)
        self.proj_impl = None    # rows -> (QKV on the MFMA kernel, o-proj on the MFMA kernel)
        self._attn_stream = None
        # called with the global layer id once that layer's KV is in the cache
        # (P/D layer-streamed migration sends finished layers while later ones compute)
        self.layer_hook = None
        self._pad_buf: Optional[torch.Tensor] = None
        self.load_info: Optional[dict] = None
        self.norms_folded = False    # fold_norms ran: in_norm / post_norm are ones, qkv / gate_up carry the gains
        self.fold_impl = None        # rows -> run the fused-norm layers? (dgi.runtime.gemm_pad)
        self._ss_buf: Optional[torch.Tensor] = None
        # "fp8" / "mxfp4": the four projections per layer are ops.Fp8Weight / ops.Mxfp4Weight
        self.weight_quant: Optional[str] = None
        self.act_quant: Optional[str] = None        # "fp8": W8A8 above ops.W8A8_MIN_M rows (quantize_weights)
        self._quant_scratch: Optional[torch.Tensor] = None
        # "fp8": a MoE model's experts_gate_up / experts_down are ops.Fp8ExpertWeight (quantize_experts)
        self.expert_quant: Optional[str] = None
        # MoE models (tests): hook(global layer, positions, ids [T, k], weights [T, k]) -> ids to
        # force, or None to keep the router's choice.  Eager steps only: it reads the routing
        self.route_hook = None
        if checkpoint:
            # real weights: only this rank's layers / TP slices are read (dgi.models.weights)
            from dgi.models.weights import load_checkpoint
            self._init_empty()
            self.load_info = load_checkpoint(self, checkpoint, getattr(self, "tp_rank", 0), getattr(self, "tp", 1))
        elif init == "random":
            self._init_random(seed)
        elif init == "empty":
            self._init_empty()
        self.cos_sin = ops.rope_cos_sin(cfg.rope_dim, cfg.max_position, cfg.rope_theta, cfg.rope_scaling,
                                        device=self.device)
        self.rope_mode = 1 if cfg.rope_interleaved else 0
        if cfg.qk_norm and self.device.type == "cuda" and \
                not ops.qknorm_rope_cache_ok(cfg.head_dim, cfg.rope_dim, self.rope_mode):
            raise ValueError(f"{cfg.name}: q/k norm on the GPU needs NeoX rotary over the whole head and head_dim "
                             f"64 or 128 (the qknorm_rope_cache kernel); got head_dim {cfg.head_dim}, rotary_dim "
                             f"{cfg.rope_dim}, {'interleaved' if self.rope_mode else 'NeoX'} pairing")

    # ------------------------------------------------------------------ weights
    def _init_empty(self):
        c, dev, dt = self.cfg, self.device, self.dtype
        H, I = c.hidden_size, c.intermediate_size
        E, Im = c.num_experts, c.moe_intermediate_size
        for _ in range(self.num_local_layers):
            self.layers.append(LlamaLayerWeights(
                torch.ones(H, device=dev, dtype=dt), torch.empty(c.qkv_size, H, device=dev, dtype=dt),
                torch.empty(H, c.q_size, device=dev, dtype=dt), torch.ones(H, device=dev, dtype=dt),
                None if c.is_moe else torch.empty(2 * I, H, device=dev, dtype=dt),
                None if c.is_moe else torch.empty(H, I, device=dev, dtype=dt),
                torch.zeros(c.qkv_size, device=dev, dtype=dt) if c.qkv_bias else None,
                torch.ones(c.head_dim, device=dev, dtype=dt) if c.qk_norm else None,
                torch.ones(c.head_dim, device=dev, dtype=dt) if c.qk_norm else None,
                torch.empty(E, H, device=dev, dtype=dt) if c.is_moe else None,
                torch.empty(E, 2 * Im, H, device=dev, dtype=dt) if c.is_moe else None,
                torch.empty(E, H, Im, device=dev, dtype=dt) if c.is_moe else None))
        if self.has_embed:
            self.embed = torch.empty(c.vocab_size, H, device=dev, dtype=dt)
        if self.has_head:
            self.norm = torch.ones(H, device=dev, dtype=dt)
            self.lm_head = self.embed if (c.tie_embeddings and self.embed is not None) else \
                torch.empty(c.vocab_size, H, device=dev, dtype=dt)

    def _init_random(self, seed: int):
        """Deterministic per-layer seeds, initialised directly on the device.

        Any rank can re-materialise its own layer range without I/O, and a
        layer's weights do not depend on how the model is sharded (SURVEY
        §5.5), so PP=k outputs equal PP=1 outputs bit for bit."""
        c, dev, dt = self.cfg, self.device, self.dtype
        H, I = c.hidden_size, c.intermediate_size
        std = 0.02
        gen = torch.Generator(device=dev)
        for li in range(self.layer_start, self.layer_end):
            gen.manual_seed(seed * 1000003 + li * 7919 + 1)
            ln1 = 1.0 + 0.1 * _rand((H,), gen, dev, torch.float32, 1.0)
            qkv = _rand((c.qkv_size, H), gen, dev, dt, std)
            o = _rand((H, c.q_size), gen, dev, dt, std / math.sqrt(2 * c.num_layers))
            ln2 = 1.0 + 0.1 * _rand((H,), gen, dev, torch.float32, 1.0)
            gu = down = None
            if not c.is_moe:
                gu = _rand((2 * I, H), gen, dev, dt, std)
                down = _rand((H, I), gen, dev, dt, std / math.sqrt(2 * c.num_layers))
            bias = _rand((c.qkv_size,), gen, dev, dt, std) if c.qkv_bias else None
            # drawn after every other tensor of the layer: models without the norm keep their weights
            qn = kn = None
            if c.qk_norm:
                qn = (1.0 + 0.1 * _rand((c.head_dim,), gen, dev, torch.float32, 1.0)).to(dt)
                kn = (1.0 + 0.1 * _rand((c.head_dim,), gen, dev, torch.float32, 1.0)).to(dt)
            # the router and the experts come last of all, so no dense model's weights move.  The
            # router's std is large enough that the experts' logits are well apart after the norm
            rt = egu = edn = None
            if c.is_moe:
                E, Im = c.num_experts, c.moe_intermediate_size
                rt = _rand((E, H), gen, dev, dt, 4 * std)
                egu = _rand((E, 2 * Im, H), gen, dev, dt, std)
                edn = _rand((E, H, Im), gen, dev, dt, std / math.sqrt(2 * c.num_layers))
            self.layers.append(LlamaLayerWeights(ln1.to(dt), qkv, o, ln2.to(dt), gu, down, bias, qn, kn,
                                                 rt, egu, edn))
        if self.has_embed or (self.has_head and c.tie_embeddings):
            gen.manual_seed(seed * 1000003 + 17)
            emb = _rand((c.vocab_size, H), gen, dev, dt, 1.0)
            self.embed = emb if self.has_embed else None
        if self.has_head:
            gen.manual_seed(seed * 1000003 + 23)
            self.norm = (1.0 + 0.1 * _rand((H,), gen, dev, torch.float32, 1.0)).to(dt)
            if c.tie_embeddings:
                self.lm_head = emb
            else:
                self.lm_head = _rand((c.vocab_size, H), gen, dev, dt, std)

    def fold_norms(self) -> None:
        """Fold each layer's RMSNorm gains into the projection that consumes the norm:
        qkv <- qkv * diag(in_norm), gate_up <- gate_up * diag(post_norm) (fp32 product,
        rounded once), and the gains become ones.  Every forward path computes the same
        function afterwards (the unfused norms multiply by ones); the fused-norm layers need
        it.  Idempotent; reloading weights clears the flag."""
        if self.norms_folded:
            return
        if self.weight_quant:
            raise RuntimeError("fold_norms: the weights are quantised; fold before quantize_weights")
        self._check_not_quantised("fold_norms")
        with torch.no_grad():
            for L in self.layers:
                for w, g in ((L.qkv, L.in_norm), (L.gate_up, L.post_norm)):
                    gf = g.float()[None]
                    step = max(1, (64 << 20) // (4 * w.shape[1]))      # bounded fp32 temporaries
                    for r0 in range(0, w.shape[0], step):
                        blk = w[r0:r0 + step]
                        blk.copy_((blk.float() * gf).to(w.dtype))
                    g.fill_(1.0)
            if self.layers and self.cfg.hidden_size % 256 == 0:
                # the row statistics of the fused-norm layers, allocated here so a graph capture
                # never allocates it (steps of more rows grow it eagerly)
                self._ss_buf = torch.zeros(16384, _ss_cols(self.cfg.hidden_size), device=self.device,
                                           dtype=torch.float32)
        self.norms_folded = True

    def quantize_weights(self, mode: str = "fp8", act_quant: Optional[str] = None) -> "LlamaModel":
        """Weight-only quantisation of each layer's qkv / o / gate_up / down projection, one layer
        at a time, dropping the bf16 tensor as it goes: ``"fp8"`` (``ops.quantize_fp8``: e4m3 codes,
        one fp32 scale per output channel) or ``"mxfp4"`` (``ops.quantize_mxfp4``: e2m1 codes, one
        e8m0 scale per 32 elements).  Norm gains (``q_norm`` / ``k_norm`` included), ``qkv_bias``,
        ``embed`` and ``lm_head`` keep their dtype.  Steps then run ``_forward_layers_quant``.

        ``act_quant="fp8"`` (W8A8, fp8 weights only) marks every quantised projection so that steps
        of at least ``ops.W8A8_MIN_M`` rows quantise their activations per token and run the e4m3
        GEMM (``ops.linear_w8a8``); smaller steps stay W8A16."""
        if mode not in ("fp8", "mxfp4"):
            raise ValueError(f"quantize_weights: unsupported mode {mode!r} (supported: 'fp8', 'mxfp4')")
        if act_quant not in (None, "fp8"):
            raise ValueError(f"quantize_weights: unsupported act_quant {act_quant!r} (supported: None, 'fp8')")
        if self.cfg.is_moe:
            raise ValueError(f"quantize_weights: {self.cfg.name} is a MoE model; its projections stay bf16, and its "
                             "experts are quantised by quantize_experts (EngineConfig.expert_quant)")
        if act_quant and mode != "fp8":
            raise ValueError(f"quantize_weights: act_quant={act_quant!r} needs mode='fp8' (the e4m3 GEMM reads "
                             f"e4m3 weights), not {mode!r}")
        if self.weight_quant == mode:
            self._set_act_quant(act_quant)
            return self
        if self.weight_quant:
            raise RuntimeError(f"quantize_weights: the model's weights are {self.weight_quant}-quantised already; "
                               f"quantise a model holding the bf16 weights to {mode!r}")
        kind, quantise = (ops.Fp8Weight, ops.quantize_fp8) if mode == "fp8" else (ops.Mxfp4Weight, ops.quantize_mxfp4)
        largest = 0
        for L in self.layers:
            for k in QUANT_SLOTS:
                w = getattr(L, k)
                if not isinstance(w, kind):
                    setattr(L, k, quantise(w))
                    del w
                N, K = getattr(L, k).shape
                largest = max(largest, N * K)
        # one bf16 buffer the size of the largest projection: the dequantised copy of the steps the
        # quantised kernel does not take (allocated here so a graph capture never allocates it)
        if largest and self.device.type == "cuda":
            self._quant_scratch = torch.empty(largest, dtype=torch.bfloat16, device=self.device)
            for L in self.layers:
                for k in QUANT_SLOTS:
                    getattr(L, k).scratch = self._quant_scratch
        self.weight_quant = mode
        self._set_act_quant(act_quant)
        if self.device.type == "cuda":
            # the KV budget reads driver-free memory: hand the freed bf16 blocks back to the driver
            torch.cuda.empty_cache()
        return self

    def _set_act_quant(self, act_quant: Optional[str]) -> None:
        if self.weight_quant == "fp8":      # mxfp4 weights have no activation mode (quantize_weights refuses one)
            for L in self.layers:
                for k in QUANT_SLOTS:
                    getattr(L, k).act = act_quant
        self.act_quant = act_quant

    def quantize_experts(self, mode: str = "fp8") -> "LlamaModel":
        """FP8 weight-only experts of a MoE model: each layer's ``experts_gate_up`` / ``experts_down``
        becomes an ``ops.Fp8ExpertWeight`` (``ops.quantize_fp8_experts``: e4m3 codes, one fp32 scale
        per expert and output channel), layer by layer, dropping the bf16 tensors as it goes.  The
        attention projections, the router, the norms and the embeddings keep their dtype; steps run
        the same ``ops.moe_mlp``, whose two GEMMs become ``moe_gemm_w8``.  Idempotent."""
        if mode == "mxfp4":
            raise ValueError("quantize_experts: 'mxfp4' is not supported for experts yet (supported: 'fp8')")
        if mode != "fp8":
            raise ValueError(f"quantize_experts: unsupported mode {mode!r} (supported: 'fp8')")
        if not self.cfg.is_moe:
            raise ValueError(f"quantize_experts: {self.cfg.name} is a dense model; quantise its projections with "
                             "quantize_weights (EngineConfig.weight_quant)")
        if self.expert_quant == mode:
            return self
        for L in self.layers:
            for k in EXPERT_SLOTS:
                w = getattr(L, k)
                if not isinstance(w, ops.Fp8ExpertWeight):
                    setattr(L, k, ops.quantize_fp8_experts(w))
                    del w
        self.expert_quant = mode
        if self.device.type == "cuda":
            # the KV budget reads driver-free memory: hand the freed bf16 blocks back to the driver
            torch.cuda.empty_cache()
        return self

    def _check_not_quantised(self, what: str) -> None:
        if self.weight_quant:
            raise RuntimeError(f"{what}: the model's weights are {self.weight_quant}-quantised; "
                               "load or copy the bf16 weights first, then call quantize_weights")
        if self.expert_quant:
            raise RuntimeError(f"{what}: the model's experts are {self.expert_quant}-quantised; "
                               "load or copy the bf16 weights first, then call quantize_experts")

    def load_state_dict_hf(self, sd: dict):
        """Load HF Llama tensor names (``model.layers.N.self_attn.q_proj.weight``...)."""
        self._check_not_quantised("load_state_dict_hf")
        self.norms_folded = False
        c = self.cfg
        for i, li in enumerate(range(self.layer_start, self.layer_end)):
            p = f"model.layers.{li}."
            L = self.layers[i]
            qkv = torch.cat([sd[p + "self_attn.q_proj.weight"], sd[p + "self_attn.k_proj.weight"],
                             sd[p + "self_attn.v_proj.weight"]], 0)
            L.qkv.copy_(qkv)
            if L.qkv_bias is not None:
                L.qkv_bias.copy_(torch.cat([sd[p + "self_attn.q_proj.bias"], sd[p + "self_attn.k_proj.bias"],
                                            sd[p + "self_attn.v_proj.bias"]], 0))
            if L.q_norm is not None:       # Qwen3: a state dict without the two gains is a KeyError
                L.q_norm.copy_(sd[p + "self_attn.q_norm.weight"])
                L.k_norm.copy_(sd[p + "self_attn.k_norm.weight"])
            L.o.copy_(sd[p + "self_attn.o_proj.weight"])
            if L.router is not None:
                self._load_experts_hf(L, sd, p + "mlp.")
            elif p + "mlp.gate_up_proj.weight" in sd:     # GLM: fused [gate; up]
                L.gate_up.copy_(sd[p + "mlp.gate_up_proj.weight"])
            else:
                L.gate_up.copy_(torch.cat([sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"]], 0))
            if L.router is None:
                L.down.copy_(sd[p + "mlp.down_proj.weight"])
            L.in_norm.copy_(sd[p + "input_layernorm.weight"])
            L.post_norm.copy_(sd[p + "post_attention_layernorm.weight"])
        if self.has_embed:
            self.embed.copy_(sd["model.embed_tokens.weight"])
        if self.has_head:
            self.norm.copy_(sd["model.norm.weight"])
            if "lm_head.weight" in sd and self.lm_head is not self.embed:
                self.lm_head.copy_(sd["lm_head.weight"])
        del c

    def _load_experts_hf(self, L: LlamaLayerWeights, sd: dict, m: str) -> None:
        """A MoE layer's router and experts from HF names under ``m`` (``model.layers.N.mlp.``): the
        fused in-memory tensors of transformers 5 (``experts.gate_up_proj [E, 2I, H]``,
        ``experts.down_proj [E, H, I]``) or the published per-expert ``experts.{e}.{gate,up,down}_proj``.
        A missing tensor is a KeyError that names it."""
        def get(name):
            if name not in sd:
                raise KeyError(f"load_state_dict_hf: {self.cfg.arch} state dict without {name}")
            return sd[name]
        L.router.copy_(get(m + "gate.weight"))
        if m + "experts.gate_up_proj" in sd:
            L.experts_gate_up.copy_(sd[m + "experts.gate_up_proj"])
            L.experts_down.copy_(get(m + "experts.down_proj"))
            return
        Im = self.cfg.moe_intermediate_size
        for e in range(self.cfg.num_experts):
            x = f"{m}experts.{e}."
            L.experts_gate_up[e, :Im].copy_(get(x + "gate_proj.weight"))
            L.experts_gate_up[e, Im:].copy_(get(x + "up_proj.weight"))
            L.experts_down[e].copy_(get(x + "down_proj.weight"))

    def tensors(self):
        """(name, tensor) pairs of every weight (lm_head omitted when tied).  A quantised
        projection yields its codes and its scales as ``<name>.q`` and ``<name>.scale``."""
        for i, L in enumerate(self.layers):
            for k in LlamaLayerWeights.__slots__:
                t = getattr(L, k)
                if isinstance(t, (ops.Fp8Weight, ops.Mxfp4Weight, ops.Fp8ExpertWeight)):
                    yield f"layers.{self.layer_start + i}.{k}.q", t.q
                    yield f"layers.{self.layer_start + i}.{k}.scale", t.scale
                elif t is not None:
                    yield f"layers.{self.layer_start + i}.{k}", t
        for k in ("embed", "norm"):
            t = getattr(self, k)
            if t is not None:
                yield k, t
        if self.lm_head is not None and self.lm_head is not self.embed:
            yield "lm_head", self.lm_head

    def copy_from(self, other: "LlamaModel") -> "LlamaModel":
        """Copy weights of the overlapping layer range from another instance
        (any device) — used to compare CPU / GPU / sharded models exactly."""
        if self.weight_quant != other.weight_quant:
            raise RuntimeError(f"copy_from: this model's weights are {self.weight_quant or 'unquantised'}, the "
                               f"source's {other.weight_quant or 'unquantised'}; copy first, then quantize_weights")
        if self.act_quant != other.act_quant:
            raise RuntimeError(f"copy_from: this model's act_quant is {self.act_quant!r}, the source's "
                               f"{other.act_quant!r}; quantize_weights both with the same act_quant")
        if self.expert_quant != other.expert_quant:
            raise RuntimeError(f"copy_from: this model's experts are {self.expert_quant or 'unquantised'}, the "
                               f"source's {other.expert_quant or 'unquantised'}; copy first, then quantize_experts")
        src = dict(other.tensors())
        self.norms_folded = other.norms_folded
        for name, t in self.tensors():
            if name in src:
                t.copy_(src[name])
        return self

    def weight_bytes(self) -> int:
        n = 0
        for L in self.layers:
            for t in (L.in_norm, L.qkv, L.o, L.post_norm, L.gate_up, L.down, L.qkv_bias, L.q_norm, L.k_norm,
                      L.router, L.experts_gate_up, L.experts_down):
                if isinstance(t, (ops.Fp8Weight, ops.Mxfp4Weight, ops.Fp8ExpertWeight)):
                    n += t.nbytes()      # codes + scales (fp8: one fp32 per row; mxfp4: one byte per 32 elements)
                elif t is not None:
                    n += t.numel() * t.element_size()
        for t in (self.embed, self.norm):
            if t is not None:
                n += t.numel() * t.element_size()
        if self.lm_head is not None and self.lm_head is not self.embed:
            n += self.lm_head.numel() * self.lm_head.element_size()
        return n

    def bind_kv(self, pool) -> None:
        """Point the model at a ``BlockPool``'s pages (and, for an fp8 pool, its scales)."""
        self.kv_cache = pool.kv
        self.kv_scale = getattr(pool, "kv_scale", None)
        self.kv_inv_scale = getattr(pool, "kv_inv_scale", None)

    @property
    def kv_fp8(self) -> bool:
        return self.kv_cache is not None and ops.is_fp8_kv(self.kv_cache)

    # ------------------------------------------------------------------ forward
    def attention(self, li: int, qkv: torch.Tensor, meta: AttnMeta, rope: bool = True,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
        c = self.cfg
        kc = self.kv_cache[li, 0]
        vc = self.kv_cache[li, 1]
        ksc = kinv = None
        if self.kv_fp8:
            if not rope:
                raise RuntimeError("fp8 KV cache: the RoPE + KV-write GEMM epilogues have no fp8 writer")
            if self.kv_scale is None or self.kv_scale.shape[0] != self.kv_cache.shape[0]:
                raise RuntimeError("fp8 KV cache without its scales: bind the pool with LlamaModel.bind_kv")
            ksc, kinv = self.kv_scale[li], self.kv_inv_scale[li]
        if c.qk_norm:
            if not rope:
                raise RuntimeError("q/k norm: the RoPE + KV-write GEMM epilogues rotate before the norm")
            L = self.layers[li]
            ops.qknorm_rope_cache(qkv, meta.positions, self.cos_sin, L.q_norm, L.k_norm, c.rms_eps, c.num_heads,
                                  c.num_kv_heads, c.head_dim, meta.slot_mapping, kc, vc, self.rope_mode,
                                  kv_inv_scale=kinv)
        elif rope:     # else the qkv GEMM epilogue already rotated q/k and wrote the cache
            ops.rope_cache(qkv, meta.positions, self.cos_sin, c.num_heads, c.num_kv_heads, c.head_dim,
                           meta.slot_mapping, kc, vc, self.rope_mode, kv_inv_scale=kinv)
        T = qkv.shape[0]
        if out is None:
            out = torch.empty(T, c.q_size, device=qkv.device, dtype=qkv.dtype)
        nd = meta.num_decode
        # this layer's sliding window (0 = full attention); a captured graph bakes it in
        window = c.window_of(self.layer_start + li)
        # mixed step: the decode rows' split-KV attention (HBM-latency bound) runs on a side
        # stream beside the prefill rows' flash attention; joined before the o-proj
        side = None
        if ATTN_OVERLAP and nd > 0 and meta.num_prefill_tokens > 0 and qkv.is_cuda \
                and not torch.cuda.is_current_stream_capturing():
            side = self._attn_stream
            if side is None or side.device != qkv.device:
                from dgi.utils.streams import named_stream
                side = self._attn_stream = named_stream("attn_side", qkv.device)
            main = torch.cuda.current_stream()
            side.wait_stream(main)
        if nd > 0:
            with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
                ops.paged_decode(qkv[:nd], kc, vc, meta.dec_block_tables, meta.dec_context_lens, c.num_heads,
                                 c.num_kv_heads, self.scale, meta.dec_max_splits, meta.dec_part_size,
                                 out=out[:nd], workspace=meta.dec_workspace, kv_scale=ksc, window=window)
        if meta.num_prefill_tokens > 0:
            ops.paged_prefill(qkv[nd:], kc, vc, meta.pre_block_tables, meta.pre_cu_seqlens, meta.pre_context_lens,
                              c.num_heads, c.num_kv_heads, self.scale, tiles=meta.pre_tiles,
                              tree_mask=meta.tree_mask, tree_n=meta.tree_n, out=out[nd:], kv_scale=ksc,
                              window=window)
        if side is not None:
            main.wait_stream(side)
        return out

    def _mlp_rows(self, T: int, like: torch.Tensor) -> int:
        """Padded MLP row count for a T-row step; sizes the buffer the o-proj writes into and
        zeroes its pad rows."""
        if self.mlp_pad is None or not like.is_cuda or torch.cuda.is_current_stream_capturing():
            return T
        Mp = self.mlp_pad(T)
        if Mp <= T:
            return T
        buf = self._pad_buf
        if buf is None or buf.shape[0] < Mp or buf.dtype != like.dtype or buf.device != like.device:
            buf = self._pad_buf = torch.empty(max(Mp, 4096), like.shape[1], dtype=like.dtype, device=like.device)
        buf[T:Mp].zero_()       # pad rows: zeros in, ignored out
        return Mp

    # ------------------------------------------------------------------ pieces the layer loops share
    def _first_norm(self, h: torch.Tensor, residual: Optional[torch.Tensor], L: LlamaLayerWeights) -> tuple:
        """A layer's input norm: (normalised h, residual stream).  Without a residual (the first
        local layer) h becomes the stream and the norm writes a fresh tensor; otherwise h is
        added into the stream and normalised in place."""
        if residual is None:
            return ops.rmsnorm(h, L.in_norm, self.cfg.rms_eps), h
        ops.fused_add_rmsnorm(h, residual, L.in_norm, self.cfg.rms_eps)
        return h, residual

    def _mlp(self, i: int, L: LlamaLayerWeights, x: torch.Tensor, positions: torch.Tensor) -> torch.Tensor:
        """Local layer ``i``'s MLP on the normalised rows ``x`` (the ``ops.linear`` route): dense
        SwiGLU, or for a MoE layer the routed experts (``ops.moe_mlp``).  ``positions`` are the rows'
        positions, for ``route_hook``."""
        if L.router is None:
            return ops.linear(ops.silu_mul(ops.linear(x, L.gate_up)), L.down)
        c = self.cfg
        k, norm = c.num_experts_per_tok, c.norm_topk_prob
        ids = None
        if self.route_hook is not None:
            if x.is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("route_hook is set during stream capture: it reads the routing, run eager steps")
            chosen, weights = ops.moe_route(ops.linear(x, L.router), k, norm)
            ids = self.route_hook(self.layer_start + i, positions, chosen, weights)
        return ops.moe_mlp(x, L.router, L.experts_gate_up, L.experts_down, k, norm, ids=ids)

    def _trimmed_tail(self, i: int, L: LlamaLayerWeights, attn: torch.Tensor, stream: torch.Tensor,
                      rows: torch.Tensor, positions: Optional[torch.Tensor] = None) -> tuple:
        """The last layer after its attention (which has written every row's K/V), on the logits
        rows ``rows`` alone: o-proj, add + norm, MLP.  Returns (MLP output, stream) of those rows;
        nothing is recorded in ``captured`` (forward() never trims while layers are captured)."""
        eps = self.cfg.rms_eps
        attn = attn.index_select(0, rows)
        stream = stream.index_select(0, rows)
        h = ops.linear(attn, L.o)
        if self.reduce is not None:
            self.reduce(h)
        ops.fused_add_rmsnorm(h, stream, L.post_norm, eps)
        h = self._mlp(i, L, h, None if positions is None else positions.index_select(0, rows))
        if self.reduce is not None:
            self.reduce(h)
        if self.layer_hook is not None:
            self.layer_hook(self.layer_start + i)
        return h, stream

    def _end_layer(self, i: int, h: torch.Tensor, residual: torch.Tensor) -> None:
        """EAGLE-3 feature tap and the layer hook of local layer ``i``."""
        li = self.layer_start + i
        if self.capture_layers and li in self.capture_layers:
            self.captured[li] = h + residual
        if self.layer_hook is not None:
            self.layer_hook(li)

    def _fused_decode(self, h: torch.Tensor, meta: AttnMeta) -> tuple:
        """(fuse qkv, fuse gate_up) for this step; (False, False) = unfused layers."""
        T, H = h.shape[0], self.cfg.hidden_size
        if meta.num_prefill_tokens != 0 and not (FUSED_SMALL_PREFILL and T <= 16):
            return False, False
        if not ((h.is_cuda and h.dtype == torch.bfloat16) or self.force_fused):
            return False, False
        # force_fused: run the fused composition through the reference ops on CPU (tests)
        if self.force_fused:
            return True, True
        return ops.fused_decode_ok(T, H, "qkv"), ops.fused_decode_ok(T, H, "gate_up")

    def _forward_layers_fused(self, h: torch.Tensor, meta: AttnMeta, residual: Optional[torch.Tensor],
                              fuse_qkv: bool = True, fuse_gu: bool = True):
        """Pure-decode layers with few rows: the qkv projection with its RMSNorm
        (+ residual add) prologue and RoPE + paged-KV epilogue in one kernel, and
        gate_up with RMSNorm prologue + SwiGLU epilogue (ops.fused_skinny,
        dgi/csrc/fused_decode.hip) — 5 kernels per layer instead of 9 when both
        are fused.  A fused prologue writes the updated residual to a fresh
        buffer (the old one is still being read by other workgroups); the
        unfused steps update it in place as forward_layers does."""
        c = self.cfg
        eps = c.rms_eps
        T = h.shape[0]
        # the RoPE + KV-write epilogue writes bf16 pages only: an fp8 pool takes the plain epilogue + rope_cache
        # (and rotates the raw projection: a model with q/k norms takes the plain epilogue + qknorm_rope_cache)
        rope_epi = (self.rope_mode == 0 and c.head_dim == 128 and self.cos_sin.shape[1] == 128 and not self.kv_fp8
                    and not c.qk_norm)
        for i, L in enumerate(self.layers):
            kc, vc = self.kv_cache[i, 0], self.kv_cache[i, 1]
            if fuse_qkv:
                qkv = torch.empty(T, L.qkv.shape[0], dtype=h.dtype, device=h.device)
                if residual is None:
                    pro, res_out, new_res = 1, None, h
                else:
                    res_out = torch.empty_like(h)
                    pro, new_res = 2, res_out
                ops.fused_skinny(qkv, h, residual, res_out, L.in_norm, eps, L.qkv, L.qkv_bias, pro,
                                 2 if rope_epi else 0, meta.positions, self.cos_sin, meta.slot_mapping, kc, vc,
                                 c.num_heads, c.num_kv_heads)
                residual = new_res
                attn = self.attention(i, qkv, meta, rope=not rope_epi)
            else:
                h, residual = self._first_norm(h, residual, L)
                attn = self.attention(i, ops.linear(h, L.qkv, L.qkv_bias), meta)
            h = ops.decode_proj(attn, L.o)
            if self.reduce is not None:
                self.reduce(h)
            if fuse_gu:
                act = torch.empty(T, L.gate_up.shape[0] // 2, dtype=h.dtype, device=h.device)
                res_out = torch.empty_like(h)
                ops.fused_skinny(act, h, residual, res_out, L.post_norm, eps, L.gate_up, None, 2, 1)
                residual = res_out
            else:
                ops.fused_add_rmsnorm(h, residual, L.post_norm, eps)
                act = ops.silu_mul(ops.linear(h, L.gate_up))
            h = ops.linear(act, L.down)
            if self.reduce is not None:
                self.reduce(h)
            self._end_layer(i, h, residual)
        return h, residual

    # ------------------------------------------------------------------ fused-norm layers
    def _fold_ok(self, h: torch.Tensor) -> bool:
        if NORM_FOLD == "0" or self.reduce is not None:
            return False
        if not h.is_cuda:           # "force-cpu": the same composition through the reference ops (tests)
            return NORM_FOLD == "force-cpu" and h.shape[0] >= NORM_FOLD_MIN_ROWS and self.layers[0].qkv_bias is None
        if h.dtype != torch.bfloat16:
            return False
        T = h.shape[0]
        if T < NORM_FOLD_MIN_ROWS:
            return False
        L = self.layers[0]
        if L.qkv_bias is not None or self.cfg.hidden_size % 256 or self.cfg.hidden_size > 8192:
            return False
        if torch.cuda.is_current_stream_capturing() and not self.norms_folded:
            return False            # weights are folded eagerly, never inside a capture
        ok = getattr(self, "_fold_shapes_ok", None)
        if ok is None:
            x = h[:1]
            a = torch.empty(1, L.o.shape[1], device=h.device, dtype=h.dtype)
            m = torch.empty(1, L.down.shape[1], device=h.device, dtype=h.dtype)
            ok = self._fold_shapes_ok = (ops.mfma_norm_ok(x, L.qkv) and ops.mfma_norm_ok(a, L.o)
                                         and ops.mfma_norm_ok(x, L.gate_up) and ops.mfma_norm_ok(m, L.down)
                                         and (L.gate_up.shape[0] // 2) % 128 == 0)
        if not ok:
            return False
        return fold_decision(NORM_FOLD, T, self.fold_impl)

    def _forward_layers_folded(self, h: torch.Tensor, meta: AttnMeta, residual: Optional[torch.Tensor],
                               trim_last: Optional[torch.Tensor]):
        """Layers on the fused-norm MFMA GEMMs (see NORM_FOLD).  Per layer::

            qkv  = rstd(ss) * (R @ qkv'^T)        (in_norm folded into qkv')
            attn = attention(qkv)
            R   += attn @ o^T;    ss <- row sums of squares of R
            act  = SwiGLU(rstd(ss) * (R @ gate_up'^T))
            R   += act @ down^T;  ss <- ...

        R is the residual stream (updated in place); returns (R, None), or for ``trim_last``
        the last layer's MLP output of the logits rows and their stream (the unfused contract)."""
        if not self.norms_folded:
            self.fold_norms()
        c = self.cfg
        eps = c.rms_eps
        T, H = h.shape
        R = h if residual is None else h + residual      # forward() hands over a tensor it owns
        nt = _ss_cols(H)
        ss = self._ss_buf
        if ss is None or ss.shape[0] < T or ss.shape[1] != nt or ss.device != h.device:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("fused-norm layers: statistics buffer must exist before capture")
            ss = self._ss_buf = torch.zeros(max(T, 4096), nt, device=h.device, dtype=torch.float32)
        ss = ss[:T]
        ops.row_sumsq(R, ss)
        n = len(self.layers)
        rope_epi = (NORM_FOLD_ROPE and (R.is_cuda or NORM_FOLD == "force-cpu") and self.rope_mode == 0 and c.head_dim == 128
                    and self.cos_sin.shape[1] == 128 and (c.num_heads * 128) % 256 == 0
                    and (c.num_kv_heads * 128) % 256 == 0 and not self.kv_fp8 and not c.qk_norm)
        for i, L in enumerate(self.layers):
            if rope_epi:
                qkv = ops.mfma_gemm_norm_rope(R, L.qkv, ss, eps, meta.positions, self.cos_sin, meta.slot_mapping,
                                              self.kv_cache[i, 0], self.kv_cache[i, 1], c.num_heads, c.num_kv_heads)
                attn = self.attention(i, qkv, meta, rope=False)
            else:
                qkv = ops.mfma_gemm_norm(R, L.qkv, ops.NORM_PLAIN, ss, eps)
                attn = self.attention(i, qkv, meta)
            if trim_last is not None and i == n - 1:
                return self._trimmed_tail(i, L, attn, R, trim_last)      # reduce is None here (_fold_ok)
            ops.mfma_gemm_norm(attn, L.o, ops.NORM_RES, ss, eps, out=R)
            act = ops.mfma_gemm_norm(R, L.gate_up, ops.NORM_SWIGLU, ss, eps)
            ops.mfma_gemm_norm(act, L.down, ops.NORM_RES, ss, eps, out=R)
            if self.capture_layers and (self.layer_start + i) in self.capture_layers:
                self.captured[self.layer_start + i] = R.clone()
            if self.layer_hook is not None:
                self.layer_hook(self.layer_start + i)
        return R, None

    def _forward_layers_quant(self, h: torch.Tensor, meta: AttnMeta, residual: Optional[torch.Tensor] = None,
                              trim_last: Optional[torch.Tensor] = None):
        """The layers of a weight-quantised model: the unfused loop with no row padding and every
        projection through ``ops.linear`` (the W8A16 kernel for decode-sized steps, dequantise +
        bf16 GEMM otherwise).  No fused-norm, fused-decode or MFMA-table layers: those read bf16
        weights."""
        return self._unfused_layers(h, meta, residual, trim_last, h.shape[0])

    def forward_layers(self, h: torch.Tensor, meta: AttnMeta, residual: Optional[torch.Tensor] = None,
                       trim_last: Optional[torch.Tensor] = None):
        """Run the local layers.  ``trim_last`` (row indices): the last layer's
        output is only needed for those rows (the rows that produce logits), so
        after its attention — which has written every row's K/V — its o-proj and
        MLP run on those rows alone and the returned (h, residual) hold just them."""
        T = h.shape[0]
        if self.weight_quant:
            return self._forward_layers_quant(h, meta, residual, trim_last)
        if not self.layers:
            return h, residual
        if self.cfg.is_moe:
            # the unfused loop, always: the fused-norm, fused-decode and MFMA-table layers read the
            # dense gate_up / down a MoE layer does not have
            return self._unfused_layers(h, meta, residual, trim_last, T)
        if self._fold_ok(h):
            return self._forward_layers_folded(h, meta, residual, trim_last)
        fq, fg = self._fused_decode(h, meta)
        if fq or fg:
            h, residual = self._forward_layers_fused(h, meta, residual, fq, fg)
            if trim_last is not None:     # same contract as the unfused path: only the logits rows
                h, residual = h.index_select(0, trim_last), residual.index_select(0, trim_last)
            return h, residual
        Mp = self._mlp_rows(T, h)
        # hand-written MFMA GEMMs where the start-up table measured them faster (dgi.runtime.gemm_pad)
        mlp = self.mlp_impl(Mp) if self.mlp_impl is not None else (False, False)
        proj = self.proj_impl(T) if (self.proj_impl is not None and h.is_cuda
                                     and not torch.cuda.is_current_stream_capturing()) else (False, False)
        return self._unfused_layers(h, meta, residual, trim_last, Mp, mlp, proj)

    def _unfused_layers(self, h: torch.Tensor, meta: AttnMeta, residual: Optional[torch.Tensor],
                        trim_last: Optional[torch.Tensor], Mp: int, mlp: tuple = (False, False),
                        proj: tuple = (False, False)):
        """norm -> QKV -> attention -> o-proj -> add + norm -> SwiGLU(gate_up) -> down, per layer.
        ``Mp`` > T: the MLP runs on Mp rows of ``_pad_buf`` (``_mlp_rows`` zeroed the pad rows) whose
        first T the o-proj writes.  ``mlp`` / ``proj``: (gate_up, down) / (QKV, o-proj) on the MFMA
        kernel rather than ``ops.linear``."""
        eps = self.cfg.rms_eps
        T = h.shape[0]
        (mfma_gu, mfma_dn), (mfma_q, mfma_o) = mlp, proj
        for i, L in enumerate(self.layers):
            h, residual = self._first_norm(h, residual, L)
            if mfma_q and L.qkv_bias is None:
                qkv = ops.mfma_gemm(h, L.qkv, 0)
            else:
                qkv = ops.linear(h, L.qkv, L.qkv_bias)
            attn = self.attention(i, qkv, meta)
            if trim_last is not None and i == len(self.layers) - 1:
                return self._trimmed_tail(i, L, attn, residual, trim_last, meta.positions)
            if Mp > T:
                # o-proj writes the first T rows of the padded MLP input
                h = ops.mfma_gemm(attn, L.o, 0, out=self._pad_buf[:T]) if mfma_o else \
                    torch.matmul(attn, L.o.t(), out=self._pad_buf[:T])
            else:
                h = ops.mfma_gemm(attn, L.o, 0) if mfma_o else ops.linear(attn, L.o)
            if self.reduce is not None:
                self.reduce(h)
            ops.fused_add_rmsnorm(h, residual, L.post_norm, eps)
            x = self._pad_buf[:Mp] if Mp > T else h
            if mfma_gu or mfma_dn:
                act = ops.mfma_gemm(x, L.gate_up, 1) if mfma_gu else ops.silu_mul(ops.linear(x, L.gate_up))
                h = ops.mfma_gemm(act, L.down, 0) if mfma_dn else ops.linear(act, L.down)
            else:
                h = self._mlp(i, L, x, meta.positions)
            if Mp > T:
                h = h[:T]
            if self.reduce is not None:
                self.reduce(h)
            self._end_layer(i, h, residual)
        return h, residual

    def embed_tokens(self, input_ids: torch.Tensor) -> torch.Tensor:
        return F.embedding(input_ids, self.embed)

    def forward(self, meta: AttnMeta, input_ids: Optional[torch.Tensor] = None,
                hidden: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Stage forward.  Returns logits [n, V] on the last stage, else the
        residual stream [T, H] for the next stage."""
        if self.has_embed:
            h = self.embed_tokens(input_ids)
        else:
            h = hidden
        residual = None
        idx = meta.logits_indices
        # the last layer's o-proj + MLP only for the rows that produce logits (prefill
        # chunks sample one row each): skipped when layers' hidden states are captured
        trim = (idx is not None and self.has_head and self.num_local_layers > 0 and TRIM_LAST_LAYER
                and not self.capture_layers and idx.shape[0] < h.shape[0])
        if self.num_local_layers:
            # a fresh residual tensor: fused_add_rmsnorm updates it in place
            h, residual = self.forward_layers(h.clone() if not self.has_embed else h, meta,
                                              trim_last=idx if trim else None)
        if not self.has_head:
            return h if residual is None else h + residual
        return self.compute_logits(h, residual, None if trim else idx)

    def compute_logits(self, h, residual, idx):
        eps = self.cfg.rms_eps
        if idx is not None:
            h = h.index_select(0, idx)
            residual = residual.index_select(0, idx) if residual is not None else None
        if residual is None:
            hn = ops.rmsnorm(h.contiguous(), self.norm, eps)
        else:
            h = h.contiguous()
            residual = residual.contiguous()
            ops.fused_add_rmsnorm(h, residual, self.norm, eps)
            hn = h
        return ops.linear(hn, self.lm_head)

    def final_hidden(self, h, residual, idx=None):
        """Normalised last hidden states (EAGLE draft features)."""
        eps = self.cfg.rms_eps
        if idx is not None:
            h = h.index_select(0, idx)
            residual = residual.index_select(0, idx)
        h = h.contiguous()
        residual = residual.contiguous().clone()
        ops.fused_add_rmsnorm(h, residual, self.norm, eps)
        return h
