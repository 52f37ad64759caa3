"""INT4 (group scale + zero point) weight-only quantisation on the CPU: the quantiser, the AWQ repack,
an AWQ checkpoint through ``load_checkpoint`` and the refusals (the GPU side: test_int4_weights_gpu.py)."""
import json
import logging

import pytest
import torch

from dgi import ops
from dgi.ops import Int4Weight, int4_from_awq, quantize_int4

AWQ_ORDER = (0, 2, 4, 6, 1, 3, 5, 7)        # AWQ "GEMM": nibble i of an int32 holds column 8c + AWQ_ORDER[i]
AWQ_CFG = {"quant_method": "awq", "bits": 4, "group_size": 128, "zero_point": True, "version": "gemm"}


def _awq_pack(v):
    """[R, C] integers 0..15 -> [R, C/8] int32, from the documented format."""
    v = v.to(torch.int64).view(v.shape[0], -1, 8)
    word = sum(v[:, :, AWQ_ORDER[i]] << (4 * i) for i in range(8))
    return torch.where(word >= 2 ** 31, word - 2 ** 32, word).to(torch.int32)


def _awq_linear(N, K, gen):
    """A random AWQ linear layer: (qweight, qzeros, scales) and its decoded [N, K] weight."""
    code = torch.randint(0, 16, (K, N), generator=gen)
    zero = torch.randint(0, 16, (K // 128, N), generator=gen)
    scale = (torch.rand(K // 128, N, generator=gen) * 0.02 + 0.001).to(torch.float16)
    w = (code - zero.repeat_interleave(128, 0)).float() * scale.float().repeat_interleave(128, 0)
    return (_awq_pack(code), _awq_pack(zero), scale), (code, zero), w.t().contiguous()


@pytest.mark.parametrize("case", ["randn", "positive", "zeros", "tiny"])
def test_quantize_int4_half_step(case):
    torch.manual_seed(1)
    w = {"randn": torch.randn(24, 512) * 0.05, "positive": torch.rand(24, 512) + 1.0, "zeros": torch.zeros(24, 512),
         "tiny": torch.randn(24, 512) * 1e-7}[case].to(torch.bfloat16)
    fw = quantize_int4(w)
    assert fw.shape == w.shape and fw.nbytes() == 24 * 512 // 2 + 24 * 4 * 4 and "24, 512" in repr(fw)
    step = fw.scales().float().repeat_interleave(128, 1)
    assert torch.isfinite(step).all() and (step > 0).all()
    # half a step, and the fp32 rounding of w / step * step
    assert ((fw.dequant() - w.float()).abs() <= step * (0.5 + 2.0 ** -20)).all()
    assert int(fw.codes().max()) <= 15 and int(fw.zeros().max()) <= 15
    with pytest.raises(ValueError, match="K % 128"):
        quantize_int4(torch.zeros(4, 192))


def test_int4_from_awq_round_trip():
    (qw, qz, sc), (code, zero), w = _awq_linear(40, 384, torch.Generator().manual_seed(2))
    fw = int4_from_awq(qw, qz, sc)
    assert fw.shape == (40, 384)
    assert torch.equal(fw.codes().long(), code.t()) and torch.equal(fw.zeros().long(), zero.t())
    assert torch.equal(fw.scales(), sc.t()) and torch.equal(fw.dequant(), w)
    # the documented layout: dword 16h + 4g + c of a row, nibble (j >> 1) + 4 (j & 1), is k = 128h + 32c + 8g + j
    for n, h, g, c, j in ((0, 0, 0, 0, 0), (5, 2, 3, 1, 7), (39, 1, 2, 3, 4), (3, 0, 1, 2, 1)):
        assert (int(fw.q[n, 16 * h + 4 * g + c]) >> (4 * ((j >> 1) + 4 * (j & 1)))) & 15 == code[128 * h + 32 * c + 8 * g + j, n]
        assert int(fw.sz[n, h]) == (0x4300 + int(zero[h, n])) << 16 | (int(sc[h, n].view(torch.int16)) & 0xFFFF)
    with pytest.raises(ValueError, match="qzeros"):
        int4_from_awq(qw, qz[:2], sc)
    with pytest.raises(ValueError, match="fp16"):
        int4_from_awq(qw, qz, sc.float())
    x = torch.randn(3, 384)
    torch.testing.assert_close(ops.linear(x, fw), x @ w.t())        # the CPU reference path


def _write_awq_checkpoint(path, mc, cfg, gen):
    """A llama-tiny AWQ checkpoint directory; returns the decoded weight of every linear layer by name."""
    from safetensors.torch import save_file
    H, I, hd = mc.hidden_size, mc.intermediate_size, mc.head_dim
    shapes = {"self_attn.q_proj": (mc.num_heads * hd, H), "self_attn.k_proj": (mc.num_kv_heads * hd, H),
              "self_attn.v_proj": (mc.num_kv_heads * hd, H), "self_attn.o_proj": (H, mc.num_heads * hd),
              "mlp.gate_proj": (I, H), "mlp.up_proj": (I, H), "mlp.down_proj": (H, I)}
    sd, decoded = {}, {}
    for li in range(mc.num_layers):
        for k, (N, K) in shapes.items():
            name = f"model.layers.{li}.{k}"
            (sd[name + ".qweight"], sd[name + ".qzeros"], sd[name + ".scales"]), _, decoded[name] = _awq_linear(N, K, gen)
        for k in ("input_layernorm", "post_attention_layernorm"):
            sd[f"model.layers.{li}.{k}.weight"] = torch.rand(H, generator=gen).to(torch.bfloat16)
    sd["model.embed_tokens.weight"] = torch.randn(mc.vocab_size, H, generator=gen).to(torch.bfloat16)
    sd["model.norm.weight"] = torch.rand(H, generator=gen).to(torch.bfloat16)
    sd["lm_head.weight"] = torch.randn(mc.vocab_size, H, generator=gen).to(torch.bfloat16)
    path.mkdir()
    save_file(sd, str(path / "model.safetensors"))
    (path / "config.json").write_text(json.dumps({"quantization_config": cfg}))
    return decoded


def test_load_awq_checkpoint(tmp_path):
    from dgi.models.config import get_config
    from dgi.models.llama import QUANT_SLOTS, LlamaModel
    from dgi.models.weights import load_checkpoint
    mc = get_config("llama-tiny-hd128")
    dec = _write_awq_checkpoint(tmp_path / "awq", mc, AWQ_CFG, torch.Generator().manual_seed(4))
    m = LlamaModel(mc, "cpu", checkpoint=str(tmp_path / "awq"))
    assert m.weight_quant == "int4" and all(isinstance(getattr(L, k), Int4Weight) for L in m.layers for k in QUANT_SLOTS)
    for li, L in enumerate(m.layers):
        a, mlp = f"model.layers.{li}.self_attn.", f"model.layers.{li}.mlp."
        assert torch.equal(L.qkv.dequant(), torch.cat([dec[a + "q_proj"], dec[a + "k_proj"], dec[a + "v_proj"]], 0))
        assert torch.equal(L.gate_up.dequant(), torch.cat([dec[mlp + "gate_proj"], dec[mlp + "up_proj"]], 0))
        assert torch.equal(L.o.dequant(), dec[a + "o_proj"]) and torch.equal(L.down.dequant(), dec[mlp + "down_proj"])
    assert m.lm_head.dtype == torch.bfloat16 and m.embed.dtype == torch.bfloat16
    # a pipeline stage reads its layers; tensor parallelism is refused; so is everything that refuses for mxfp4
    stage = LlamaModel(mc, "cpu", layer_start=1, has_embed=False, checkpoint=str(tmp_path / "awq"))
    assert torch.equal(stage.layers[0].down.q, m.layers[1].down.q) and "layers.1.qkv.sz" in dict(stage.tensors())
    with pytest.raises(ValueError, match="tensor parallelism"):
        load_checkpoint(LlamaModel(mc, "cpu", init="empty"), str(tmp_path / "awq"), 0, 2)
    assert m.quantize_weights("int4") is m
    for call, err in ((lambda: m.quantize_weights("mxfp4"), "int4-quantised"), (m.fold_norms, "quantised"),
                      (lambda: m.copy_from(LlamaModel(mc, "cpu")), "quantize_weights"),
                      (lambda: load_checkpoint(m, str(tmp_path / "awq")), "quantised")):
        with pytest.raises(RuntimeError, match=err):
            call()
    with pytest.raises(ValueError, match="act_quant"):
        LlamaModel(mc, "cpu").quantize_weights("int4", act_quant="fp8")


@pytest.mark.parametrize("change", [{"quant_method": "gptq"}, {"bits": 8}, {"group_size": 64}, {"zero_point": False},
                                    {"version": "gemv"}])
def test_other_quantised_checkpoints_are_refused(change, tmp_path):
    from dgi.models.weights import checkpoint_quantization
    (tmp_path / "config.json").write_text(json.dumps({"quantization_config": {**AWQ_CFG, **change}}))
    with pytest.raises(ValueError, match="bits 4, group_size 128, zero_point true and version 'gemm'"):
        checkpoint_quantization(str(tmp_path))


@pytest.mark.parametrize("value,expect", [("awq", "int4"), ("AWQ", "int4"), ("gptq", None), ("int8", None)])
def test_public_switches(value, expect, caplog):
    """The switches spell the mode "awq" (the reference's name; "int4" stays an unknown value to them)."""
    from dgi.engine import EngineConfig
    from engines.llm_native import NativeLLMEngine
    assert EngineConfig(weight_quant="awq").weight_quant == "awq"
    assert ops.skinny_i4_cfg_ok(ops._skinny_i4_cfg(17, 28672, 4096), 28672, 4096) and not ops.skinny_i4_cfg_ok(3, 256, 1024)
    e = NativeLLMEngine({"model_id": "llama-tiny", "device": "cpu", "max_model_len": 256, "num_blocks": 64,
                         "max_num_seqs": 4, "quantization": value})
    with caplog.at_level(logging.INFO, logger="engines.llm_native"):
        e.load_model()
    try:
        assert e.engine.model.weight_quant == expect and e.engine.cfg.weight_quant == (expect and "awq")
        assert any("not supported" in r.getMessage() for r in caplog.records) == (expect is None)
        assert any("not AWQ's" in r.getMessage() for r in caplog.records) == (expect == "int4")
    finally:
        e.unload_model()
