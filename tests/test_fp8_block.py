"""Block-scaled FP8 (128 x 128 scales) on the CPU: the repack to 16-row tiles, what ``checkpoint_quantization``
accepts, the loader's refusals and a checkpoint round trip (the GPU side: test_fp8_block_gpu.py)."""
import json

import pytest
import torch

from dgi import ops
from dgi.ops import Fp8BlockWeight, fp8_block_cat, fp8_block_from_hf

FP8_CFG = {"quant_method": "fp8", "fmt": "e4m3", "weight_block_size": [128, 128], "activation_scheme": "dynamic",
           "modules_to_not_convert": ["lm_head"]}


def _hf_linear(N, K, gen):
    """Random codes and block scales in the checkpoint's shapes, and the [N, K] weight they define."""
    q = (torch.randn(N, K, generator=gen) * 100).clamp_(-448, 448).to(torch.float8_e4m3fn)
    s = torch.rand((N + 127) // 128, (K + 127) // 128, generator=gen) * 0.01 + 0.001
    w = q.float() * s.repeat_interleave(128, 0)[:N].repeat_interleave(128, 1)[:, :K]
    return q, s, w


def test_from_hf_and_cat():
    gen = torch.Generator().manual_seed(0)
    parts, dec = [], []
    for N in (256, 192, 128):           # 192: the second 128-row block is partial, and the next part starts inside it
        q, s, w = _hf_linear(N, 384, gen)
        fw = fp8_block_from_hf(q, s)
        assert fw.scale.shape == (N // 16, 3) and torch.equal(fw.dequant(), w)
        parts.append(fw)
        dec.append(w)
    qkv = fp8_block_cat(parts)
    assert qkv.shape == (576, 384) and qkv.nbytes() == 576 * 384 + 4 * 36 * 3
    assert torch.equal(qkv.dequant(), torch.cat(dec, 0))
    x = torch.randn(3, 384, generator=gen)
    torch.testing.assert_close(ops.linear(x, qkv), x @ torch.cat(dec, 0).t())       # the CPU reference path
    q, s, _ = _hf_linear(256, 384, gen)
    for call, err in ((lambda: fp8_block_from_hf(q, s, block=(64, 64)), "128, 128"),
                      (lambda: fp8_block_from_hf(q.view(torch.uint8), s), "float8_e4m3fn"),
                      (lambda: fp8_block_from_hf(q, s.double()), "float32"),
                      (lambda: fp8_block_from_hf(q, s[:1]), "blocks"),
                      (lambda: fp8_block_from_hf(q[:, :192].contiguous(), s[:, :2].contiguous()), "K % 128"),
                      (lambda: Fp8BlockWeight(q[:24], s.repeat_interleave(8, 0)[:2]), "N % 16")):
        with pytest.raises(ValueError, match=err):
            call()


@pytest.mark.parametrize("change,ok", [({}, True), ({"fmt": None, "activation_scheme": None}, True),
                                       ({"weight_block_size": None}, False), ({"weight_block_size": [64, 64]}, False),
                                       ({"activation_scheme": "static"}, False), ({"fmt": "e5m2"}, False)])
def test_checkpoint_quantization(change, ok, tmp_path):
    from dgi.models.weights import checkpoint_quantization
    qc = {k: v for k, v in {**FP8_CFG, **change}.items() if v is not None}
    (tmp_path / "config.json").write_text(json.dumps({"quantization_config": qc}))
    if ok:
        assert checkpoint_quantization(str(tmp_path)) == "fp8_block"
    else:
        with pytest.raises(ValueError, match=r"version 'gemm', and quant_method 'fp8' .* \[128, 128\]"):
            checkpoint_quantization(str(tmp_path))


def _write_checkpoint(path, mc, gen, H=None, keep=()):
    """A block-FP8 checkpoint of ``mc`` (``H``: a hidden size for the weights other than the config's);
    returns the decoded weight of every linear layer by name, and its (codes, block scales).  Layers in
    ``keep`` are written in bf16."""
    from safetensors.torch import save_file
    H, I, hd = H or mc.hidden_size, mc.intermediate_size, mc.head_dim
    shapes = {"self_attn.q_proj": (mc.num_heads * hd, H), "self_attn.k_proj": (mc.num_kv_heads * hd, H),
              "self_attn.v_proj": (mc.num_kv_heads * hd, H), "self_attn.o_proj": (H, mc.num_heads * hd),
              "mlp.gate_proj": (I, H), "mlp.up_proj": (I, H), "mlp.down_proj": (H, I)}
    sd, dec, raw = {}, {}, {}
    for li in range(mc.num_layers):
        for k, (N, K) in shapes.items():
            name = f"model.layers.{li}.{k}"
            q, s, dec[name] = _hf_linear(N, K, gen)
            raw[name] = (q, s)
            if name in keep:
                sd[name + ".weight"] = dec[name] = dec[name].to(torch.bfloat16)
            else:
                sd[name + ".weight"], sd[name + ".weight_scale_inv"] = q, s
        for k in ("input_layernorm", "post_attention_layernorm"):
            sd[f"model.layers.{li}.{k}.weight"] = torch.rand(H, generator=gen).to(torch.bfloat16)
    sd["model.embed_tokens.weight"] = torch.randn(mc.vocab_size, H, generator=gen).to(torch.bfloat16)
    sd["model.norm.weight"] = torch.rand(H, generator=gen).to(torch.bfloat16)
    sd["lm_head.weight"] = torch.randn(mc.vocab_size, H, generator=gen).to(torch.bfloat16)
    path.mkdir()
    save_file(sd, str(path / "model.safetensors"))
    (path / "config.json").write_text(json.dumps({"quantization_config": {**FP8_CFG, "modules_to_not_convert":
                                                                          ["lm_head", *keep]}}))
    return dec, raw


def test_load_checkpoint_round_trip(tmp_path):
    from dgi.engine import EngineConfig, LLMEngine
    from dgi.models.config import get_config
    from dgi.models.llama import QUANT_SLOTS, LlamaModel
    from dgi.sched.request import SamplingParams
    mc = get_config("llama-tiny-hd128")
    path = tmp_path / "fp8"
    dec, raw = _write_checkpoint(path, mc, torch.Generator().manual_seed(4), keep=("model.layers.1.mlp.down_proj",))
    m = LlamaModel(mc, "cpu", checkpoint=str(path))
    assert m.weight_quant == "fp8" and m.act_quant is None and m.lm_head.dtype == torch.bfloat16
    # the same model put together by hand: codes as written, each block row repeated for its 16-row tiles
    ref = LlamaModel(mc, "cpu", init="empty")
    for name, t in m.tensors():
        if not name.endswith((".q", ".scale")):
            dict(ref.tensors())[name].copy_(t)
    for li, (L, R) in enumerate(zip(m.layers, ref.layers)):
        a, mlp = f"model.layers.{li}.self_attn.", f"model.layers.{li}.mlp."
        slots = {"qkv": [a + "q_proj", a + "k_proj", a + "v_proj"], "o": [a + "o_proj"],
                 "gate_up": [mlp + "gate_proj", mlp + "up_proj"], "down": [mlp + "down_proj"]}
        for k in QUANT_SLOTS:
            w, want = getattr(L, k), torch.cat([dec[n] for n in slots[k]], 0)
            if (li, k) == (1, "down"):          # listed in modules_to_not_convert: read as bf16, stays a tensor
                assert w.dtype == torch.bfloat16 and torch.equal(w, want)
                continue
            assert isinstance(w, Fp8BlockWeight) and torch.equal(w.dequant(), want)
            setattr(R, k, Fp8BlockWeight(torch.cat([raw[n][0] for n in slots[k]], 0), torch.cat(
                [raw[n][1].repeat_interleave(8, 0)[:raw[n][0].shape[0] // 16] for n in slots[k]], 0)))
    ref._adopt_quantised("fp8", Fp8BlockWeight)
    assert m.weight_bytes() < 0.6 * LlamaModel(mc, "cpu", init="empty").weight_bytes()
    assert m.quantize_weights("fp8") is m            # a no-op, as on any fp8 model
    with pytest.raises(RuntimeError, match="fp8-quantised already"):
        m.quantize_weights("mxfp4")
    with pytest.raises(RuntimeError, match="quantised"):
        m.fold_norms()
    # the CPU engine over the loaded checkpoint serves linear_fp8_block_ref of those containers
    sp = SamplingParams(max_tokens=6, temperature=0.0, ignore_eos=True)
    outs = []
    for model in (m, ref):
        eng = LLMEngine(EngineConfig(model=mc.name, device="cpu", num_blocks=64, max_num_seqs=4, max_model_len=128,
                                     max_num_batched_tokens=64, use_graphs=False, weight_quant="fp8"),
                        model_cfg=mc, model=model)
        outs.append([r.output for r in eng.generate([[1, 7, 8, 9], [1, 30, 31]], sp)])
    assert outs[0] == outs[1] and all(len(o) == 6 for o in outs[0])


def test_loader_refusals(tmp_path):
    from dgi.engine import EngineConfig, LLMEngine
    from dgi.models.config import get_config
    from dgi.models.llama import LlamaModel
    from dgi.models.weights import load_checkpoint
    mc = get_config("llama-tiny-hd128")
    gen = torch.Generator().manual_seed(5)
    _write_checkpoint(tmp_path / "fp8", mc, gen)
    path = str(tmp_path / "fp8")
    with pytest.raises(ValueError, match="tensor parallelism"):
        load_checkpoint(LlamaModel(mc, "cpu", init="empty"), path, 0, 2)
    with pytest.raises(ValueError, match="MoE"):
        load_checkpoint(LlamaModel(get_config("qwen3-moe-tiny"), "cpu", init="empty"), path)
    with pytest.raises(ValueError, match="act_quant.*per-channel"):
        LLMEngine(EngineConfig(model=mc.name, device="cpu", num_blocks=64, max_model_len=128, use_graphs=False,
                               weight_quant="fp8", act_quant="fp8"), model_cfg=mc, model=LlamaModel(mc, "cpu", checkpoint=path))
    # a hidden size of 1088 = 8.5 blocks: K is no multiple of 128
    _write_checkpoint(tmp_path / "k", mc, gen, H=1088)
    with pytest.raises(ValueError, match="K % 128"):
        LlamaModel(mc, "cpu", checkpoint=str(tmp_path / "k"))
    # a bf16 linear layer that modules_to_not_convert does not list
    _write_checkpoint(tmp_path / "bf", mc, gen, keep=("model.layers.0.self_attn.o_proj",))
    (tmp_path / "bf" / "config.json").write_text(json.dumps({"quantization_config": FP8_CFG}))
    with pytest.raises(ValueError, match="o_proj.weight is torch.bfloat16"):
        LlamaModel(mc, "cpu", checkpoint=str(tmp_path / "bf"))
