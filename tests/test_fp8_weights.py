"""FP8 weight-only quantisation: the quantiser, the reference linear, the quantised model path
of a CPU engine and the configuration plumbing (the GPU kernels: test_fp8_weights_gpu.py)."""
import logging

import pytest
import torch
import torch.nn.functional as F

from dgi import ops
from dgi.ops import Fp8Weight, quantize_fp8

PROMPTS = [[1] + list(range(7, 7 + n - 1)) for n in (5, 40, 200, 7)]


@pytest.fixture(scope="module")
def quantised():
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(1152, 2048, generator=g) * 0.05).to(torch.bfloat16)
    w[17].zero_()
    w[300] = (w[300].float() * 2.0 ** -6).to(torch.bfloat16)
    return w, quantize_fp8(w)


def test_quantiser_format(quantised):
    w, fw = quantised
    assert isinstance(fw, Fp8Weight)
    assert fw.q.dtype == torch.float8_e4m3fn and fw.q.shape == w.shape and fw.q.is_contiguous()
    assert fw.scale.dtype == torch.float32 and fw.scale.shape == (w.shape[0],)
    assert fw.shape == w.shape and fw.device == w.device
    assert fw.dequant(torch.bfloat16).dtype == torch.bfloat16


def test_quantiser_codes_and_scales(quantised):
    w, fw = quantised
    qf = fw.q.float()
    assert torch.isfinite(qf).all()
    nz = torch.ones(w.shape[0], dtype=torch.bool)
    nz[17] = False
    assert torch.equal(qf.abs().amax(dim=1)[nz], torch.full((w.shape[0] - 1,), 448.0))
    assert torch.equal(fw.scale[nz], w.float().abs().amax(dim=1)[nz] / 448)
    assert float(fw.scale[17]) == 1.0
    assert torch.count_nonzero(fw.dequant(torch.float32)[17]) == 0


def test_quantiser_error_bound(quantised):
    w, fw = quantised
    wf = w.float()
    err = (fw.dequant(torch.float32) - wf).abs()
    # half an ulp of a 3-bit mantissa | half the smallest subnormal; 1e-6: the fp32 divide and multiply
    bound = torch.maximum(wf.abs() * 2.0 ** -4, fw.scale[:, None] * 2.0 ** -10) * (1 + 1e-6)
    ratio = float((err / bound.clamp_min(1e-30)).max())
    print("max error / bound:", ratio)
    assert (err <= bound).all(), ratio


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("with_out", [False, True])
def test_reference_linear_bit_exact(quantised, dtype, with_bias, with_out):
    _w, fw = quantised
    g = torch.Generator().manual_seed(1)
    x = torch.randn(5, 2048, generator=g).to(dtype)
    bias = torch.randn(1152, generator=g).to(dtype) if with_bias else None
    ref = F.linear(x.float(), fw.q.float() * fw.scale[:, None], None if bias is None else bias.float()).to(x.dtype)
    out = torch.full((5, 1152), float("nan"), dtype=dtype) if with_out else None
    y = ops.linear(x, fw, bias, out)
    if with_out:
        assert y is out
    assert y.dtype == dtype and torch.equal(y, ref)


def _engine(weight_quant=None, model=None):
    from dgi.engine import EngineConfig, LLMEngine
    from dgi.models.config import get_config
    return LLMEngine(EngineConfig(model="llama-tiny-hd128", device="cpu", dtype=torch.float32, num_blocks=256,
                                  max_num_seqs=8, max_model_len=512, max_num_batched_tokens=256, use_graphs=False,
                                  seed=3, weight_quant=weight_quant),
                     model_cfg=get_config("llama-tiny-hd128"), model=model)


def test_cpu_engine_matches_dequantised_model(monkeypatch):
    from dgi.models.llama import QUANT_SLOTS, LlamaModel
    from dgi.sched.request import SamplingParams
    calls = {"quant": 0, "other": []}
    orig = LlamaModel._forward_layers_quant

    def spy(self, *a, **k):
        calls["quant"] += 1
        return orig(self, *a, **k)
    monkeypatch.setattr(LlamaModel, "_forward_layers_quant", spy)
    for name in ("_forward_layers_folded", "_forward_layers_fused", "_mlp_rows", "fold_norms"):
        def other(self, *a, _n=name, _o=getattr(LlamaModel, name), **k):
            calls["other"].append((_n, self.weight_quant))
            return _o(self, *a, **k)
        monkeypatch.setattr(LlamaModel, name, other)

    qe = _engine("fp8")
    qm = qe.model
    assert qm.weight_quant == "fp8" and qm._quant_scratch is None        # CPU: no dequant scratch
    expect = 0
    for L in qm.layers:
        for k in QUANT_SLOTS:
            fw = getattr(L, k)
            assert isinstance(fw, Fp8Weight)
            expect += fw.q.numel() + 4 * fw.q.shape[0]
        expect += 4 * (L.in_norm.numel() + L.post_norm.numel())
        assert L.qkv_bias is None
    expect += 4 * (qm.embed.numel() + qm.norm.numel())
    if qm.lm_head is not qm.embed:
        expect += 4 * qm.lm_head.numel()
    assert qm.weight_bytes() == expect
    assert qm.embed.dtype == torch.float32 and qm.lm_head.dtype == torch.float32

    # the other engine: same seed, its projections overwritten with the dequantised fp32 weights
    re_ = _engine(None)
    assert re_.model.weight_quant is None
    assert re_.model.weight_bytes() > qm.weight_bytes()
    for L, Lq in zip(re_.model.layers, qm.layers):
        for k in QUANT_SLOTS:
            w = getattr(L, k)
            fw = quantize_fp8(w)
            assert torch.equal(fw.q.view(torch.uint8), getattr(Lq, k).q.view(torch.uint8))
            w.copy_(fw.dequant(torch.float32))

    sp = SamplingParams(max_tokens=10, temperature=0.0, ignore_eos=True)
    calls["quant"] = 0
    calls["other"].clear()
    got = [r.output for r in qe.generate(PROMPTS, sp)]
    assert calls["quant"] > 0
    assert calls["other"] == [], calls["other"]          # no other layer path ran on the quantised model
    want = [r.output for r in re_.generate(PROMPTS, sp)]
    assert all(len(o) == 10 for o in got)
    assert got == want


def test_engine_quantises_a_passed_model_once():
    from dgi.models.config import get_config
    from dgi.models.llama import LlamaModel
    m = LlamaModel(get_config("llama-tiny-hd128"), "cpu", torch.float32, seed=3)
    e = _engine("fp8", model=m)
    assert e.model is m and m.weight_quant == "fp8"
    q0 = m.layers[0].qkv.q
    e2 = _engine("fp8", model=m)                # already quantised: left alone
    assert e2.model.layers[0].qkv.q is q0


def test_quantised_model_tensors_and_copy_from():
    from dgi.models.config import get_config
    from dgi.models.llama import LlamaModel
    mc = get_config("llama-tiny-hd128")
    m = LlamaModel(mc, "cpu", torch.float32, seed=3).quantize_weights("fp8")
    names = dict(m.tensors())
    assert names["layers.0.qkv.q"].dtype == torch.float8_e4m3fn
    assert names["layers.0.qkv.scale"].dtype == torch.float32
    plain = LlamaModel(mc, "cpu", torch.float32, seed=4)
    with pytest.raises(RuntimeError, match="quantize_weights"):
        plain.copy_from(m)
    with pytest.raises(RuntimeError, match="quantize_weights"):
        m.copy_from(plain)
    with pytest.raises(RuntimeError, match="quantised"):
        m.fold_norms()
    with pytest.raises(RuntimeError, match="quantised"):
        m.load_state_dict_hf({})
    with pytest.raises(ValueError, match="fp8"):
        plain.quantize_weights("int8")
    m2 = LlamaModel(mc, "cpu", torch.float32, seed=4).quantize_weights("fp8").copy_from(m)
    assert torch.equal(m2.layers[1].down.q.view(torch.uint8), m.layers[1].down.q.view(torch.uint8))
    assert torch.equal(m2.layers[1].down.scale, m.layers[1].down.scale)


def test_engine_config_rejects_unknown_quant():
    from dgi.engine import EngineConfig
    with pytest.raises(ValueError, match="int4"):
        EngineConfig(weight_quant="int4")
    assert EngineConfig().weight_quant is None
    cfg = EngineConfig(weight_quant="fp8")
    # the pipeline and P/D engines copy the config field by field
    assert EngineConfig(**{**cfg.__dict__, "device": "cpu"}).weight_quant == "fp8"


def test_skinny_w8_cfg_table():
    assert set(ops.SKINNY_W8_CFGS) == set(range(1, 9))
    assert ops.skinny_w8_cfg_ok(0, 96, 1024) and ops.skinny_w8_cfg_ok(1, 256, 14336)
    assert not ops.skinny_w8_cfg_ok(5, 1168, 1024)        # two column tiles per wave: N % 32
    assert not ops.skinny_w8_cfg_ok(7, 256, 1024)         # 16 waves: K % 2048
    assert not ops.skinny_w8_cfg_ok(8, 96, 1024)          # four column tiles per wave: N % 64
    assert not ops.skinny_w8_cfg_ok(1, 256, 3584)


@pytest.mark.parametrize("key,value,expect", [("quantization", "fp8", "fp8"), ("weight_quant", "fp8", "fp8"),
                                              ("quantization", "int8", None)])
def test_native_worker_quantization_key(key, value, expect, caplog):
    from engines.llm_native import NativeLLMEngine
    e = NativeLLMEngine({"model_id": "llama-tiny", "device": "cpu", "max_model_len": 256, "num_blocks": 64,
                         "max_num_seqs": 4, key: value})
    with caplog.at_level(logging.WARNING, logger="engines.llm_native"):
        e.load_model()
    try:
        assert e.engine.model.weight_quant == expect
        assert e.engine.cfg.weight_quant == expect
        warned = [r for r in caplog.records if "quantization" in r.getMessage() and "fp8" in r.getMessage()]
        assert bool(warned) == (expect is None)
    finally:
        e.unload_model()


def test_node_flag_reaches_engine_config():
    from dgi.serve import node
    seen = {}

    class Stop(Exception):
        pass

    def fake_router(args, fabric, layout):
        seen["wq"] = args.weight_quant
        raise Stop
    orig, node.Router = node.Router, fake_router
    try:
        for argv, want in ((["--weight-quant", "fp8"], "fp8"), ([], None)):
            with pytest.raises(Stop):
                node.main(argv)
            assert seen["wq"] == want
        with pytest.raises(SystemExit):
            node.main(["--weight-quant", "int4"])
    finally:
        node.Router = orig
