"""Model configurations (Llama-3 8B/70B, Mistral-7B, Qwen2.5 7B/0.5B, Qwen3 0.6B/8B/32B, Qwen3-30B-A3B (MoE), GLM-4-9B, OPT-125m, tiny test models).

Mirrors the fields the reference reads from HF ``AutoConfig``
(worker/distributed/model_shard.py:273-311 uses hidden_size,
num_attention_heads, num_key_value_heads, intermediate_size,
num_hidden_layers) so ``ShardedModelLoader`` and the native runtime share one
description.  No network: presets are built in; ``from_hf_dict`` accepts a
local ``config.json`` dictionary.
"""
from __future__ import annotations

import dataclasses
import json
import os
import re
from typing import Optional


@dataclasses.dataclass
class ModelConfig:
    name: str
    arch: str = "llama"  # "llama" | "qwen2" | "qwen3" | "qwen3_moe" | "glm" | "opt"
    vocab_size: int = 128256
    hidden_size: int = 4096
    intermediate_size: int = 14336
    num_layers: int = 32
    num_heads: int = 32
    num_kv_heads: int = 8
    head_dim: int = 128
    rope_theta: float = 500000.0
    rope_scaling: Optional[dict] = None
    rms_eps: float = 1e-5
    max_position: int = 8192
    tie_embeddings: bool = False
    qkv_bias: bool = False          # Qwen2 / GLM-4: biased q/k/v projections
    rotary_dim: Optional[int] = None  # rotated dims per head (GLM-4: head_dim / 2); None = head_dim
    rope_interleaved: bool = False  # GLM-4 / GPT-J pairing (2i, 2i+1) instead of NeoX (i, i+rd/2)
    qk_norm: bool = False           # Qwen3: RMSNorm over each q and k head (gain [head_dim]) before RoPE
    bos_token_id: int = 128000
    eos_token_id: int = 128001
    # Qwen3-MoE: every layer's MLP is num_experts_per_tok of num_experts SwiGLU experts of width
    # moe_intermediate_size (no shared expert); num_experts == 0 is a dense model
    num_experts: int = 0
    num_experts_per_tok: int = 0
    moe_intermediate_size: int = 0
    norm_topk_prob: bool = False      # renormalise the k chosen probabilities to sum to one
    # Sliding-window attention (Mistral, Qwen2): a query at position p of a windowed layer sees keys
    # j with p - sliding_window < j <= p (HF's rule); 0 = every layer attends over the whole context.
    # window_layers: the global indices of the layers that slide; None with a window means all.
    sliding_window: int = 0
    window_layers: Optional[tuple] = None

    def window_of(self, global_layer: int) -> int:
        """The window of layer ``global_layer`` (index in the whole model); 0 = full attention."""
        if self.sliding_window <= 0:
            return 0
        if self.window_layers is None or global_layer in self.window_layers:
            return self.sliding_window
        return 0

    @property
    def has_window(self) -> bool:
        return any(self.window_of(li) for li in range(self.num_layers))

    @property
    def is_moe(self) -> bool:
        return self.num_experts > 0

    @property
    def rope_dim(self) -> int:
        return self.rotary_dim or self.head_dim

    @property
    def q_size(self) -> int:
        return self.num_heads * self.head_dim

    @property
    def kv_size(self) -> int:
        return self.num_kv_heads * self.head_dim

    @property
    def qkv_size(self) -> int:
        return self.q_size + 2 * self.kv_size

    def param_count(self) -> int:
        H, I, V, L = self.hidden_size, self.intermediate_size, self.vocab_size, self.num_layers
        mlp = 2 * H * I + I * H
        if self.is_moe:     # the router and the experts' gate, up and down
            mlp = self.num_experts * (H + 3 * H * self.moe_intermediate_size)
        per_layer = H * self.qkv_size + self.q_size * H + mlp + 2 * H
        if self.qkv_bias:
            per_layer += self.qkv_size
        if self.qk_norm:
            per_layer += 2 * self.head_dim
        emb = V * H * (1 if self.tie_embeddings else 2)
        return L * per_layer + emb + H

    def kv_bytes_per_token(self, dtype_bytes: int = 2, layers: Optional[int] = None) -> int:
        L = self.num_layers if layers is None else layers
        return 2 * L * self.num_kv_heads * self.head_dim * dtype_bytes

    def to_dict(self) -> dict:
        return dataclasses.asdict(self)

    @staticmethod
    def from_hf_dict(d: dict, name: str = "hf") -> "ModelConfig":
        mt = d.get("model_type", "llama")
        if mt == "opt":
            H = d["hidden_size"]
            nh = d["num_attention_heads"]
            return ModelConfig(name=name, arch="opt", vocab_size=d["vocab_size"], hidden_size=H,
                               intermediate_size=d.get("ffn_dim", 4 * H), num_layers=d["num_hidden_layers"],
                               num_heads=nh, num_kv_heads=nh, head_dim=H // nh,
                               max_position=d.get("max_position_embeddings", 2048),
                               tie_embeddings=True, bos_token_id=d.get("bos_token_id", 2),
                               eos_token_id=d.get("eos_token_id", 2), rms_eps=1e-5)
        H = d["hidden_size"]
        nh = d["num_attention_heads"]
        # transformers >= 5 nests RoPE settings under ``rope_parameters``
        rp = d.get("rope_parameters") or {}
        theta = d.get("rope_theta", rp.get("rope_theta", 10000.0))
        scaling = d.get("rope_scaling")
        if scaling is None and rp.get("rope_type", "default") != "default":
            scaling = dict(rp)
        eos = d.get("eos_token_id", 2)
        if isinstance(eos, list):
            eos = eos[0]
        arch = {"qwen2": "qwen2", "qwen3": "qwen3", "qwen3_moe": "qwen3_moe", "glm": "glm"}.get(mt, "llama")
        moe = {}
        if mt == "qwen3_moe":
            # the published files say num_experts; transformers 5 save_pretrained writes num_local_experts
            ne = d.get("num_experts") or d.get("num_local_experts")
            if not ne:
                raise ValueError(f"{name}: qwen3_moe config without num_experts / num_local_experts")
            # every layer must be sparse: a dense layer served through the experts (or the reverse)
            # would be silently wrong
            if d.get("decoder_sparse_step", 1) != 1:
                raise ValueError(f"{name}: Qwen3-MoE with decoder_sparse_step="
                                 f"{d.get('decoder_sparse_step')} is not supported (every layer must be sparse)")
            if d.get("mlp_only_layers"):
                raise ValueError(f"{name}: Qwen3-MoE with mlp_only_layers={d.get('mlp_only_layers')} is not "
                                 f"supported (mixed dense / sparse layers)")
            moe = dict(num_experts=int(ne), num_experts_per_tok=int(d["num_experts_per_tok"]),
                       moe_intermediate_size=int(d["moe_intermediate_size"]),
                       norm_topk_prob=bool(d.get("norm_topk_prob", False)))
        if mt in ("qwen3", "qwen3_moe"):
            # every layer must attend over the whole context: a sliding-window layer served as a
            # full-attention one would be silently wrong
            if d.get("use_sliding_window"):
                raise ValueError(f"{name}: Qwen3 with use_sliding_window is not supported")
            bad = sorted({t for t in (d.get("layer_types") or []) if t != "full_attention"})
            if bad:
                raise ValueError(f"{name}: Qwen3 layer_types {bad} are not supported (full_attention only)")
        # Mistral slides on every layer, Qwen2 (with use_sliding_window) on layers >= max_window_layers;
        # an explicit layer_types list wins for both
        win = {}
        if mt in ("mistral", "qwen2"):
            L = d["num_hidden_layers"]
            W = int(d.get("sliding_window") or 0)
            if W < 0:
                raise ValueError(f"{name}: sliding_window {W} is negative")
            lt = d.get("layer_types")
            if lt:
                bad = sorted({t for t in lt if t not in ("full_attention", "sliding_attention")})
                if bad or len(lt) != L:
                    raise ValueError(f"{name}: layer_types must name full_attention / sliding_attention for each "
                                     f"of the {L} layers, got {lt}")
                slide = tuple(i for i, t in enumerate(lt) if t == "sliding_attention")
                if slide and W == 0:
                    raise ValueError(f"{name}: sliding_attention layers without a sliding_window")
            elif mt == "mistral":
                slide = tuple(range(L)) if W else ()
            else:
                slide = tuple(range(int(d.get("max_window_layers", L)), L)) if d.get("use_sliding_window") and W else ()
            if slide:
                win = dict(sliding_window=W, window_layers=None if len(slide) == L else slide)
        hd = d.get("head_dim") or H // nh
        prf = d.get("partial_rotary_factor", rp.get("partial_rotary_factor", 1.0))
        rot = int(hd * prf) if prf and prf < 1.0 else None
        return ModelConfig(name=name, arch=arch, vocab_size=d["vocab_size"], hidden_size=H,
                           intermediate_size=d.get("intermediate_size", 0) if moe else d["intermediate_size"],
                           num_layers=d["num_hidden_layers"],
                           num_heads=nh, num_kv_heads=d.get("num_key_value_heads", nh),
                           head_dim=d.get("head_dim") or H // nh, rope_theta=float(theta),
                           rope_scaling=scaling, rms_eps=d.get("rms_norm_eps", 1e-5),
                           max_position=d.get("max_position_embeddings", 8192),
                           tie_embeddings=d.get("tie_word_embeddings", False),
                           qkv_bias=bool(d.get("attention_bias", mt == "qwen2")),
                           rotary_dim=rot, rope_interleaved=(mt == "glm"),
                           qk_norm=(mt in ("qwen3", "qwen3_moe")), bos_token_id=d.get("bos_token_id", 1),
                           eos_token_id=eos, **moe, **win)

    @staticmethod
    def from_file(path: str) -> "ModelConfig":
        if os.path.isdir(path):
            path = os.path.join(path, "config.json")
        with open(path) as f:
            return ModelConfig.from_hf_dict(json.load(f), name=os.path.basename(os.path.dirname(path)))


PRESETS: dict[str, ModelConfig] = {
    "llama3-8b": ModelConfig(name="llama3-8b"),
    "llama3-70b": ModelConfig(name="llama3-70b", hidden_size=8192, intermediate_size=28672, num_layers=80,
                              num_heads=64, num_kv_heads=8),
    # Small but shape-faithful (GQA 8:1, head_dim 128) Llama for tests / smoke.
    "llama-tiny": ModelConfig(name="llama-tiny", vocab_size=512, hidden_size=512, intermediate_size=1024,
                              num_layers=2, num_heads=8, num_kv_heads=1, head_dim=64, max_position=2048,
                              bos_token_id=1, eos_token_id=2),
    "llama-tiny-hd128": ModelConfig(name="llama-tiny-hd128", vocab_size=1024, hidden_size=1024,
                                    intermediate_size=2048, num_layers=4, num_heads=8, num_kv_heads=1,
                                    head_dim=128, max_position=4096, bos_token_id=1, eos_token_id=2),
    # GQA with 2 KV heads so tensor parallelism of degree 2 has a head per rank
    "llama-tiny-tp": ModelConfig(name="llama-tiny-tp", vocab_size=1024, hidden_size=1024, intermediate_size=2048,
                                 num_layers=2, num_heads=8, num_kv_heads=2, head_dim=128, max_position=4096,
                                 bos_token_id=1, eos_token_id=2),
    # Mistral-7B-v0.1: the Llama block with a 4096-token sliding window on every layer.  Shapes as the
    # published config is remembered; it could not be checked offline, and a local config.json always
    # takes precedence.
    "mistral-7b": ModelConfig(name="mistral-7b", vocab_size=32000, hidden_size=4096, intermediate_size=14336,
                              num_layers=32, num_heads=32, num_kv_heads=8, head_dim=128, rope_theta=10000.0,
                              rms_eps=1e-5, max_position=32768, sliding_window=4096, bos_token_id=1,
                              eos_token_id=2),
    # tiny Mistral for tests: a 40-token window on both layers
    "mistral-tiny": ModelConfig(name="mistral-tiny", vocab_size=1024, hidden_size=1024, intermediate_size=2048,
                                num_layers=2, num_heads=8, num_kv_heads=2, head_dim=128, rope_theta=10000.0,
                                max_position=4096, sliding_window=40, bos_token_id=1, eos_token_id=2),
    # Qwen2 / Qwen2.5 family (the reference's default LLM is Qwen2.5-7B-Instruct):
    # Llama block + biased QKV, GQA 7:1 (7B) / 7:1 (0.5B), theta 1e6
    "qwen2.5-7b": ModelConfig(name="qwen2.5-7b", arch="qwen2", vocab_size=152064, hidden_size=3584,
                              intermediate_size=18944, num_layers=28, num_heads=28, num_kv_heads=4, head_dim=128,
                              rope_theta=1000000.0, rms_eps=1e-6, max_position=32768, qkv_bias=True,
                              bos_token_id=151643, eos_token_id=151645),
    "qwen2.5-0.5b": ModelConfig(name="qwen2.5-0.5b", arch="qwen2", vocab_size=151936, hidden_size=896,
                                intermediate_size=4864, num_layers=24, num_heads=14, num_kv_heads=2, head_dim=64,
                                rope_theta=1000000.0, rms_eps=1e-6, max_position=32768, tie_embeddings=True,
                                qkv_bias=True, bos_token_id=151643, eos_token_id=151645),
    # shape-faithful tiny Qwen2 (biased QKV, GQA 7:1, tied embeddings) for tests
    "qwen-tiny": ModelConfig(name="qwen-tiny", arch="qwen2", vocab_size=1024, hidden_size=1024,
                             intermediate_size=1536, num_layers=2, num_heads=14, num_kv_heads=2, head_dim=128,
                             rope_theta=1000000.0, rms_eps=1e-6, max_position=4096, tie_embeddings=True,
                             qkv_bias=True, bos_token_id=1, eos_token_id=2),
    # qwen-tiny with a 40-token window on layer 1 only (Qwen2's max_window_layers = 1)
    "qwen-tiny-swa": ModelConfig(name="qwen-tiny-swa", arch="qwen2", vocab_size=1024, hidden_size=1024,
                                 intermediate_size=1536, num_layers=2, num_heads=14, num_kv_heads=2, head_dim=128,
                                 rope_theta=1000000.0, rms_eps=1e-6, max_position=4096, tie_embeddings=True,
                                 qkv_bias=True, sliding_window=40, window_layers=(1,), bos_token_id=1,
                                 eos_token_id=2),
    # Qwen3 dense family: the Llama block with no QKV bias, an explicit head_dim of 128 (q_size !=
    # hidden_size on 0.6B and 32B) and an RMSNorm over each q / k head before RoPE.  Shapes as the
    # published configs are remembered; they could not be checked offline, and a local config.json
    # always takes precedence (get_config reads a path before it guesses from a name).
    "qwen3-8b": ModelConfig(name="qwen3-8b", arch="qwen3", vocab_size=151936, hidden_size=4096,
                            intermediate_size=12288, num_layers=36, num_heads=32, num_kv_heads=8, head_dim=128,
                            rope_theta=1000000.0, rms_eps=1e-6, max_position=40960, qk_norm=True,
                            bos_token_id=151643, eos_token_id=151645),
    "qwen3-32b": ModelConfig(name="qwen3-32b", arch="qwen3", vocab_size=151936, hidden_size=5120,
                             intermediate_size=25600, num_layers=64, num_heads=64, num_kv_heads=8, head_dim=128,
                             rope_theta=1000000.0, rms_eps=1e-6, max_position=40960, qk_norm=True,
                             bos_token_id=151643, eos_token_id=151645),
    "qwen3-0.6b": ModelConfig(name="qwen3-0.6b", arch="qwen3", vocab_size=151936, hidden_size=1024,
                              intermediate_size=3072, num_layers=28, num_heads=16, num_kv_heads=8, head_dim=128,
                              rope_theta=1000000.0, rms_eps=1e-6, max_position=40960, tie_embeddings=True,
                              qk_norm=True, bos_token_id=151643, eos_token_id=151645),
    # tiny Qwen3 for tests: q_size = 2 * hidden_size on purpose, 2 KV heads (TP=2 has one per rank)
    "qwen3-tiny": ModelConfig(name="qwen3-tiny", arch="qwen3", vocab_size=1024, hidden_size=1024,
                              intermediate_size=2048, num_layers=2, num_heads=16, num_kv_heads=2, head_dim=128,
                              rope_theta=1000000.0, rms_eps=1e-6, max_position=4096, tie_embeddings=True,
                              qk_norm=True, bos_token_id=1, eos_token_id=2),
    # Qwen3-MoE: the Qwen3 attention block with a top-k routed set of SwiGLU experts as every layer's
    # MLP.  Qwen3-30B-A3B as its published config is remembered (not checkable offline; a local
    # config.json takes precedence).  intermediate_size is the config's dense width, which no layer uses.
    "qwen3-30b-a3b": ModelConfig(name="qwen3-30b-a3b", arch="qwen3_moe", vocab_size=151936, hidden_size=2048,
                                 intermediate_size=6144, num_layers=48, num_heads=32, num_kv_heads=4, head_dim=128,
                                 rope_theta=1000000.0, rms_eps=1e-6, max_position=40960, qk_norm=True,
                                 bos_token_id=151643, eos_token_id=151645, num_experts=128,
                                 num_experts_per_tok=8, moe_intermediate_size=768, norm_topk_prob=True),
    # tiny Qwen3-MoE for tests: 8 experts of width 256, 2 per token
    "qwen3-moe-tiny": ModelConfig(name="qwen3-moe-tiny", arch="qwen3_moe", vocab_size=1024, hidden_size=512,
                                  intermediate_size=1024, num_layers=2, num_heads=8, num_kv_heads=2, head_dim=128,
                                  rope_theta=1000000.0, rms_eps=1e-6, max_position=4096, qk_norm=True,
                                  bos_token_id=1, eos_token_id=2, num_experts=8, num_experts_per_tok=2,
                                  moe_intermediate_size=256, norm_topk_prob=True),
    # GLM-4-9B (HF "glm"): Llama block + biased QKV, GQA 16:1, half-dim interleaved RoPE
    "glm-4-9b": ModelConfig(name="glm-4-9b", arch="glm", vocab_size=151552, hidden_size=4096,
                            intermediate_size=13696, num_layers=40, num_heads=32, num_kv_heads=2, head_dim=128,
                            rope_theta=10000.0, rms_eps=1.5625e-07, max_position=131072, qkv_bias=True,
                            rotary_dim=64, rope_interleaved=True, bos_token_id=151331, eos_token_id=151329),
    "glm-tiny": ModelConfig(name="glm-tiny", arch="glm", vocab_size=1024, hidden_size=1024, intermediate_size=1536,
                            num_layers=2, num_heads=8, num_kv_heads=2, head_dim=128, rope_theta=10000.0,
                            rms_eps=1.5625e-07, max_position=4096, qkv_bias=True, rotary_dim=64,
                            rope_interleaved=True, bos_token_id=1, eos_token_id=2),
    "opt-125m": ModelConfig(name="opt-125m", arch="opt", vocab_size=50272, hidden_size=768,
                            intermediate_size=3072, num_layers=12, num_heads=12, num_kv_heads=12, head_dim=64,
                            max_position=2048, tie_embeddings=True, bos_token_id=2, eos_token_id=2),
}

ALIASES = {
    "meta-llama/Meta-Llama-3-8B": "llama3-8b",
    "meta-llama/Meta-Llama-3-8B-Instruct": "llama3-8b",
    "meta-llama/Llama-3.1-8B-Instruct": "llama3-8b",
    "meta-llama/Meta-Llama-3-70B": "llama3-70b",
    "meta-llama/Meta-Llama-3-70B-Instruct": "llama3-70b",
    "mistralai/Mistral-7B-v0.1": "mistral-7b",
    "facebook/opt-125m": "opt-125m",
    "Qwen/Qwen2.5-7B-Instruct": "qwen2.5-7b",
    "Qwen/Qwen2.5-7B": "qwen2.5-7b",
    "Qwen/Qwen2-7B-Instruct": "qwen2.5-7b",
    "Qwen/Qwen2.5-0.5B-Instruct": "qwen2.5-0.5b",
    "Qwen/Qwen3-8B": "qwen3-8b",
    "Qwen/Qwen3-32B": "qwen3-32b",
    "Qwen/Qwen3-0.6B": "qwen3-0.6b",
    "THUDM/glm-4-9b-chat-hf": "glm-4-9b",
    "THUDM/glm-4-9b-chat": "glm-4-9b",
    "THUDM/glm-4-9b-hf": "glm-4-9b",
}


def get_config(name_or_path: str) -> ModelConfig:
    """Preset, alias, HF config dir/file, or a family guess from the name.
    ``<model>@L<n>`` keeps the architecture and truncates it to ``n`` layers
    (multi-rank rehearsals of a big model's shapes on one GPU); sliding-window layers keep
    their windows by global index."""
    if "@L" in name_or_path:
        base, n = name_or_path.rsplit("@L", 1)
        return dataclasses.replace(get_config(base), name=name_or_path, num_layers=int(n))
    key = ALIASES.get(name_or_path, name_or_path)
    if key in PRESETS:
        return dataclasses.replace(PRESETS[key])
    if os.path.exists(name_or_path):
        return ModelConfig.from_file(name_or_path)
    lk = key.lower()
    if "glm-4" in lk or "glm4" in lk:
        return dataclasses.replace(PRESETS["glm-4-9b"], name=name_or_path)
    if "qwen3" in lk:
        # the size comes from the name; a size without a preset (the MoE models, "-A3B", included)
        # is an error, never a guess
        tail = lk.split("qwen3", 1)[1]
        if not re.search(r"-a\d+(\.\d+)?b", tail):
            for size in ("0.6b", "32b", "8b"):
                if re.search(rf"(?<![\d.]){re.escape(size)}(?![\d])", tail):
                    return dataclasses.replace(PRESETS["qwen3-" + size], name=name_or_path)
        hint = " (Qwen3-30B-A3B is the preset 'qwen3-30b-a3b')" if re.search(r"30b-a3b", tail) else ""
        raise KeyError(f"unknown Qwen3 model {name_or_path!r}: presets exist for "
                       f"{sorted(k for k in PRESETS if k.startswith('qwen3-'))}; pass a preset key or a local "
                       f"config.json{hint}")
    if "qwen" in lk:
        return dataclasses.replace(PRESETS["qwen2.5-0.5b" if "0.5b" in lk else "qwen2.5-7b"], name=name_or_path)
    if "70b" in lk:
        return dataclasses.replace(PRESETS["llama3-70b"], name=name_or_path)
    if "8b" in lk or "7b" in lk:
        return dataclasses.replace(PRESETS["llama3-8b"], name=name_or_path)
    raise KeyError(f"unknown model {name_or_path!r}; presets: {sorted(PRESETS)}")
