"""FP8 W8A8 projections on the CPU: the row quantiser's formula, the reference projection, the
routing of ``ops.linear``, and the ``act_quant`` knob from the serving flags down to the model
(the kernels: test_w8a8_gpu.py)."""
import logging
import os
import sys

import pytest
import torch

from dgi import ops
from dgi.ops import Fp8Weight, quantize_fp8

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "worker"))

PROMPTS = [[1] + list(range(7, 7 + n - 1)) for n in (5, 40)]


def _weight(N, K, seed=0):
    g = torch.Generator().manual_seed(seed)
    return quantize_fp8(torch.randn(N, K, generator=g) * 0.05)


def test_quant_rows_ref_values():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(9, 64, generator=g) * torch.exp2(torch.arange(9.) - 4)[:, None]
    x[4] = 0
    for xin in (x, x.to(torch.bfloat16)):
        q, sx = ops.quant_rows_fp8_ref(xin)
        assert q.dtype == torch.float8_e4m3fn and q.shape == x.shape
        assert sx.dtype == torch.float32 and sx.shape == (9,)
        qf, xf = q.float(), xin.float()
        assert bool((qf.abs() <= 448).all())
        amax = xf.abs().amax(1)
        for m in range(9):
            if m == 4:
                continue
            k = int(xf[m].abs().argmax())
            assert float(qf[m, k]) == (448.0 if xf[m, k] > 0 else -448.0)
            # sx * 448 == amax to within 1 ulp
            back = sx[m] * 448
            ulp = torch.nextafter(amax[m], torch.tensor(float("inf"))) - amax[m]
            assert abs(float(back - amax[m])) <= float(ulp)
        assert float(sx[4]) == 1.0 and not qf[4].any()
    # the kernel's entry point is the reference off the GPU
    q2, s2 = ops.quant_rows_fp8(x)
    q1, s1 = ops.quant_rows_fp8_ref(x)
    assert torch.equal(q2.view(torch.uint8), q1.view(torch.uint8)) and torch.equal(s2, s1)


def test_quant_rows_ref_round_trip():
    """A row of e4m3-exact values times a power of two comes back exactly."""
    codes = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    codes = codes[(codes != 0x7F) & (codes != 0xFF)]
    vals = codes.view(torch.float8_e4m3fn).float()           # every finite e4m3 value, +-448 included
    for e in (-6, 0, 5):
        x = (vals * 2.0 ** e)[None, :]
        q, sx = ops.quant_rows_fp8_ref(x)
        assert float(sx[0]) == 2.0 ** e
        assert torch.equal(q.float() * sx[:, None], x)


def test_linear_w8a8_ref_is_linear_of_dequantised():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(5, 256, generator=g)
    w = _weight(48, 256)
    b = torch.randn(48, generator=g)
    q, sx = ops.quant_rows_fp8_ref(x)
    xd = q.float() * sx[:, None]
    for bias in (None, b):
        want = ops.linear(xd, w.dequant(torch.float32), bias)
        got = ops.linear_w8a8_ref(x, w, bias)
        torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)
        assert torch.equal(ops.linear_w8a8(x, w, bias), got)     # off the GPU: the reference
    out = torch.empty(5, 48)
    assert ops.linear_w8a8(x, w, b, out) is out and torch.equal(out, ops.linear_w8a8_ref(x, w, b))


def test_fp8weight_act_slot():
    w = _weight(16, 64)
    assert w.act is None
    assert Fp8Weight(w.q, w.scale, None).act is None            # constructor positions unchanged
    assert Fp8Weight(w.q, w.scale, None, "fp8").act == "fp8"
    assert Fp8Weight(w.q, w.scale, act="fp8").scratch is None
    with pytest.raises(ValueError, match="act"):
        Fp8Weight(w.q, w.scale, act="int8")


def test_linear_routing_cpu(monkeypatch):
    assert ops.W8A8_MIN_M == int(os.environ.get("DGI_W8A8_MIN_M", "2048"))
    monkeypatch.setattr(ops, "W8A8_MIN_M", 33)
    g = torch.Generator().manual_seed(3)
    w = _weight(48, 256)
    wa = Fp8Weight(w.q, w.scale, act="fp8")
    b = torch.randn(48, generator=g)
    calls = []
    orig = ops.linear_w8a8_ref

    def spy(x, w_, bias=None):
        calls.append(x.shape[0])
        return orig(x, w_, bias)
    monkeypatch.setattr(ops, "linear_w8a8_ref", spy)
    x40, x8 = torch.randn(40, 256, generator=g), torch.randn(8, 256, generator=g)
    y40 = ops.linear(x40, wa, b)
    assert calls == [40] and torch.equal(y40, orig(x40, wa, b))
    y8 = ops.linear(x8, wa, b)
    assert calls == [40] and torch.equal(y8, ops.linear_fp8_ref(x8, w, b))
    # act=None: today's results at both row counts, bit for bit
    for x in (x40, x8):
        assert torch.equal(ops.linear(x, w, b), ops.linear_fp8_ref(x, w, b))
    assert calls == [40]
    # the W8A8 result is a different function of x (it quantises the activations)
    assert not torch.equal(y40, ops.linear_fp8_ref(x40, w, b))
    monkeypatch.setattr(ops, "W8A8_MIN_M", 1)
    ops.linear(x8, wa, b)
    assert calls == [40, 8]


def test_engine_config_act_quant():
    from dgi.engine import ACT_QUANT_MODES, EngineConfig
    assert ACT_QUANT_MODES == (None, "fp8")
    assert EngineConfig().act_quant is None and EngineConfig(weight_quant="fp8").act_quant is None
    cfg = EngineConfig(weight_quant="fp8", act_quant="fp8")
    assert EngineConfig(**{**cfg.__dict__, "device": "cpu"}).act_quant == "fp8"
    with pytest.raises(ValueError, match="weight_quant"):
        EngineConfig(act_quant="fp8")
    with pytest.raises(ValueError, match="int8"):
        EngineConfig(weight_quant="fp8", act_quant="int8")


def test_model_act_quant():
    from dgi.models.config import get_config
    from dgi.models.llama import QUANT_SLOTS, LlamaModel
    mc = get_config("llama-tiny-hd128")
    m = LlamaModel(mc, "cpu", torch.float32, seed=3).quantize_weights("fp8", act_quant="fp8")
    assert m.weight_quant == "fp8" and m.act_quant == "fp8"
    assert all(getattr(L, k).act == "fp8" for L in m.layers for k in QUANT_SLOTS)
    plain = LlamaModel(mc, "cpu", torch.float32, seed=4).quantize_weights("fp8")
    assert plain.act_quant is None
    assert all(getattr(L, k).act is None for L in plain.layers for k in QUANT_SLOTS)
    with pytest.raises(RuntimeError, match="act_quant"):
        plain.copy_from(m)
    with pytest.raises(RuntimeError, match="act_quant"):
        m.copy_from(plain)
    with pytest.raises(ValueError, match="act_quant"):
        LlamaModel(mc, "cpu", torch.float32, seed=4).quantize_weights("fp8", act_quant="int8")
    m2 = LlamaModel(mc, "cpu", torch.float32, seed=4).quantize_weights("fp8", act_quant="fp8").copy_from(m)
    assert torch.equal(m2.layers[1].down.q.view(torch.uint8), m.layers[1].down.q.view(torch.uint8))
    # the knob of an already quantised model can be turned without re-quantising
    codes = plain.layers[0].qkv.q
    plain.quantize_weights("fp8", act_quant="fp8")
    assert plain.act_quant == "fp8" and plain.layers[0].qkv.q is codes and plain.layers[0].qkv.act == "fp8"


@pytest.mark.parametrize("extra,expect", [({"quantization": "fp8", "act_quant": "fp8"}, ("fp8", "fp8")),
                                          ({"quantization": "fp8"}, ("fp8", None)),
                                          ({"act_quant": "fp8"}, (None, None))])
def test_native_worker_act_quant_key(extra, expect, caplog):
    from engines.llm_native import NativeLLMEngine
    e = NativeLLMEngine({"model_id": "llama-tiny", "device": "cpu", "max_model_len": 256, "num_blocks": 64,
                         "max_num_seqs": 4, **extra})
    with caplog.at_level(logging.WARNING, logger="engines.llm_native"):
        e.load_model()
    try:
        assert (e.engine.cfg.weight_quant, e.engine.cfg.act_quant) == expect
        assert (e.engine.model.weight_quant, e.engine.model.act_quant) == expect
        warned = [r for r in caplog.records if "act_quant" in r.getMessage()]
        assert bool(warned) == ("quantization" not in extra)
    finally:
        e.unload_model()


def test_node_flag_reaches_engine_config():
    from dgi.serve import node
    seen = {}

    class Stop(Exception):
        pass

    def fake_router(args, fabric, layout):
        seen["aq"] = args.act_quant
        raise Stop
    orig, node.Router = node.Router, fake_router
    try:
        for argv, want in ((["--weight-quant", "fp8", "--act-quant", "fp8"], "fp8"), (["--weight-quant", "fp8"], None)):
            with pytest.raises(Stop):
                node.main(argv)
            assert seen["aq"] == want
        with pytest.raises(SystemExit):
            node.main(["--weight-quant", "fp8", "--act-quant", "int8"])
    finally:
        node.Router = orig


def _generate(act_quant):
    from dgi.engine import EngineConfig, LLMEngine
    from dgi.sched.request import SamplingParams
    eng = LLMEngine(EngineConfig(model="llama-tiny-hd128", device="cpu", dtype=torch.float32, num_blocks=64,
                                 max_num_seqs=4, max_model_len=256, max_num_batched_tokens=64, use_graphs=False,
                                 enable_prefix_caching=False, weight_quant="fp8", act_quant=act_quant, seed=11))
    assert eng.model.act_quant == act_quant
    sp = SamplingParams(max_tokens=8, temperature=0.0, ignore_eos=True)
    return [r.output for r in eng.generate(PROMPTS, sp)]


def test_cpu_engine_w8a8(monkeypatch):
    """Deterministic, and with the threshold above every step's row count exactly the W8A16 engine."""
    monkeypatch.setattr(ops, "W8A8_MIN_M", 1)
    calls = []
    orig = ops.linear_w8a8_ref

    def spy(x, w_, bias=None):
        calls.append(x.shape[0])
        return orig(x, w_, bias)
    monkeypatch.setattr(ops, "linear_w8a8_ref", spy)
    a = _generate("fp8")
    n = len(calls)
    assert n > 0 and all(len(o) == 8 for o in a)
    assert _generate("fp8") == a
    plain = _generate(None)
    assert len(calls) == 2 * n                       # act_quant=None never takes the W8A8 path
    monkeypatch.setattr(ops, "W8A8_MIN_M", 1 << 20)
    assert _generate("fp8") == plain
    assert len(calls) == 2 * n
