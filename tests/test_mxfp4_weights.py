"""MXFP4 weight-only quantisation: the format, the quantiser, the reference linear, the quantised
model path of a CPU engine and the configuration plumbing (the GPU kernels:
test_mxfp4_weights_gpu.py).  The oracle is the OCP e2m1 table, written out here."""
import logging

import pytest
import torch
import torch.nn.functional as F

from dgi import ops
from dgi.ops import Mxfp4Weight, quantize_mxfp4

PROMPTS = [[1] + list(range(7, 7 + n - 1)) for n in (5, 40, 200, 7)]
# OCP MX v1.0, e2m1: magnitude by code 0..7; bit 3 is the sign
GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
TABLE = torch.tensor(GRID + tuple(-v for v in GRID), dtype=torch.float64)


def _decode(fw):
    """The weight in float64 from the table above: low nibble first, 2^(scale - 127) per 32 elements."""
    q = fw.q.cpu()
    N, K = q.shape[0], 2 * q.shape[1]
    codes = torch.stack((q & 15, q >> 4), dim=-1).reshape(N, K).long()
    s = torch.exp2(fw.scale.cpu().double() - 127).repeat_interleave(32, dim=1)
    return TABLE[codes] * s


@pytest.fixture(scope="module")
def quantised():
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(1152, 2048, generator=g) * 0.05).to(torch.bfloat16)
    w[17].zero_()
    w[300] = (w[300].float() * 2.0 ** -6).to(torch.bfloat16)
    return w, quantize_mxfp4(w)


def test_format(quantised):
    w, fw = quantised
    assert fw.q.dtype == torch.uint8 and fw.q.shape == (1152, 1024) and fw.q.is_contiguous()
    assert fw.scale.dtype == torch.uint8 and fw.scale.shape == (1152, 64) and fw.scale.is_contiguous()
    assert fw.shape == (1152, 2048) and fw.device == w.device
    assert fw.nbytes() == 1152 * 1024 + 1152 * 64
    assert fw.scratch is None
    for dt in (torch.float32, torch.bfloat16):
        d = fw.dequant(dt)
        assert d.dtype == dt and d.shape == (1152, 2048)
        assert torch.equal(d.double(), _decode(fw))           # every value is a bf16 number
    assert not fw.dequant()[17].any()


def test_nibble_order_and_scale():
    """A hand-built 1 x 32 block: element 2j is the low nibble of byte j, 2j + 1 the high one."""
    q = torch.zeros(1, 16, dtype=torch.uint8)
    q[0, 0] = 0x21          # elements 0, 1 = codes 1, 2 = 0.5, 1
    q[0, 1] = 0xF7          # elements 2, 3 = codes 7, 15 = 6, -6
    q[0, 15] = 0x9C         # elements 30, 31 = codes 12, 9 = -2, -0.5
    for code, factor in ((127, 1.0), (130, 8.0), (120, 2.0 ** -7), (2, 2.0 ** -125), (252, 2.0 ** 125)):
        d = Mxfp4Weight(q, torch.full((1, 1), code, dtype=torch.uint8)).dequant()
        want = torch.zeros(32)
        want[:4] = torch.tensor([0.5, 1.0, 6.0, -6.0])
        want[30:] = torch.tensor([-2.0, -0.5])
        assert torch.equal(d[0], want * factor)
    # all 16 codes
    q = (torch.arange(16, dtype=torch.uint8) | ((15 - torch.arange(16, dtype=torch.uint8)) << 4))[None]
    d = Mxfp4Weight(q.contiguous(), torch.full((1, 1), 127, dtype=torch.uint8)).dequant()[0].double()
    assert torch.equal(d[0::2], TABLE) and torch.equal(d[1::2], TABLE.flip(0))


def test_constructor_rejects():
    q = torch.zeros(4, 32, dtype=torch.uint8)
    s = torch.full((4, 2), 127, dtype=torch.uint8)
    Mxfp4Weight(q, s)
    for bad_q, bad_s in ((q.to(torch.int8), s), (q, s.float()), (q, s[:, :1].contiguous()), (q, s[:3]),
                         (q.view(-1), s), (torch.zeros(4, 64, dtype=torch.uint8)[:, ::2], s),
                         (q, torch.full((4, 4), 127, dtype=torch.uint8)[:, ::2]),
                         (torch.zeros(4, 24, dtype=torch.uint8), torch.full((4, 1), 127, dtype=torch.uint8))):
        with pytest.raises(ValueError, match="Mxfp4Weight"):
            Mxfp4Weight(bad_q, bad_s)
    with pytest.raises(ValueError, match="quantize_mxfp4"):
        quantize_mxfp4(torch.zeros(4, 48))
    with pytest.raises(ValueError, match="quantize_mxfp4"):
        quantize_mxfp4(torch.zeros(64))


def test_quantiser_ties():
    """Ties go to the code whose mantissa bit is 0, in units of the block scale; the sign is kept."""
    ties = [(0.25, 0.0), (0.75, 1.0), (1.25, 1.0), (1.75, 2.0), (2.5, 2.0), (3.5, 4.0), (5.0, 4.0)]
    for j in (-20, 0, 9):
        w = torch.zeros(2, 32)
        w[:, 0] = 6.0                       # pins the block exponent at j
        for i, (v, _) in enumerate(ties):
            w[0, 1 + i] = v
            w[1, 1 + i] = -v
        w[0, 20], w[1, 20] = 0.0, -0.0
        fw = quantize_mxfp4(w * 2.0 ** j)
        assert fw.scale.tolist() == [[127 + j], [127 + j]]
        d = fw.dequant() * 2.0 ** -j
        want = torch.tensor([t for _, t in ties])
        assert torch.equal(d[0, 1:8], want) and torch.equal(d[1, 1:8], -want)
        codes = torch.stack((fw.q & 15, fw.q >> 4), dim=-1).reshape(2, 32)
        assert codes[0, 1:8].tolist() == [0, 2, 2, 4, 4, 6, 6]
        assert codes[1, 1:8].tolist() == [8, 10, 10, 12, 12, 14, 14]       # -0.25 -> -0
        assert codes[0, 20] == 0 and codes[1, 20] == 8                      # -0 keeps its sign


def test_quantiser_zero_block_and_exponent():
    w = torch.zeros(3, 64)
    w[1, 40] = 1.0
    fw = quantize_mxfp4(w)
    assert fw.scale[0].tolist() == [127, 127] and fw.scale[1, 0] == 127 and fw.scale[2].tolist() == [127, 127]
    assert not fw.q[0].any() and not fw.dequant()[0].any()
    # amax at 6 * 2^j, one ulp above and one below: the smallest exponent that does not saturate
    for j in (-30, -1, 0, 5, 40):
        top = torch.tensor(6.0 * 2.0 ** j)
        above = torch.nextafter(top, torch.tensor(float("inf")))
        below = torch.nextafter(top, torch.tensor(0.0))
        w = torch.zeros(3, 32)
        w[0, 3], w[1, 3], w[2, 3] = top, -above, below
        fw = quantize_mxfp4(w)
        assert fw.scale[:, 0].tolist() == [127 + j, 128 + j, 127 + j]
        d = fw.dequant()
        assert d[0, 3] == top and d[1, 3] == -3.0 * 2.0 ** (j + 1) and d[2, 3] == top
    # amax at every grid point times 2^j: representable exactly at the chosen exponent
    for g in GRID[1:]:
        w = torch.zeros(1, 32)
        w[0, 31] = g * 2.0 ** -3
        fw = quantize_mxfp4(w)
        assert fw.dequant()[0, 31] == g * 2.0 ** -3
        E = int(fw.scale[0, 0]) - 127
        assert g * 2.0 ** -3 <= 6.0 * 2.0 ** E and g * 2.0 ** -3 > 6.0 * 2.0 ** (E - 1)


def test_quantiser_nearest_grid_point():
    """Per-block magnitudes spread over 2^+-20: every element lands on a nearest grid point."""
    g = torch.Generator().manual_seed(2)
    w = torch.randn(64, 1024, generator=g)
    mag = torch.exp2(torch.randint(-20, 21, (64, 32), generator=g).float())
    w = (w.view(64, 32, 32) * mag[:, :, None]).view(64, 1024)
    fw = quantize_mxfp4(w)
    assert int(fw.scale.min()) >= 2 and int(fw.scale.max()) <= 252
    wd = w.double()
    err = (wd - _decode(fw)).abs()
    s = torch.exp2(fw.scale.double() - 127).repeat_interleave(32, dim=1)
    for gv in TABLE.tolist()[:8] + TABLE.tolist()[9:]:            # the 15 distinct signed grid values
        assert bool((err <= (wd - gv * s).abs()).all()), gv
    # nothing saturates: every block's amax is within the grid
    assert bool((wd.abs() <= 6.0 * s).all())
    # and the scale is the smallest such
    amax = wd.abs().view(64, 32, 32).amax(dim=2)
    assert bool((amax > 3.0 * torch.exp2(fw.scale.double() - 127)).all())


def test_quantiser_code_range():
    """Blocks far outside the scale range clamp to codes 2 and 252 (saturating or flushing)."""
    w = torch.zeros(2, 32)
    w[0, 0], w[0, 1] = 3.0e38, -1.0e38
    w[1, 0] = 1.0e-44
    fw = quantize_mxfp4(w)
    assert fw.scale[:, 0].tolist() == [252, 2]
    d = fw.dequant()
    assert d[0, 0] == 6.0 * 2.0 ** 125 and d[0, 1] < 0 and torch.isfinite(d).all() and d[1, 0] == 0


def test_quantiser_dtype_independent(quantised):
    w, fw = quantised
    f32 = quantize_mxfp4(w.float())
    assert torch.equal(f32.q, fw.q) and torch.equal(f32.scale, fw.scale)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("with_out", [False, True])
def test_reference_linear_bit_exact(quantised, dtype, with_bias, with_out):
    _w, fw = quantised
    g = torch.Generator().manual_seed(1)
    x = torch.randn(5, 2048, generator=g).to(dtype)
    bias = torch.randn(1152, generator=g).to(dtype) if with_bias else None
    ref = F.linear(x.float(), fw.dequant(torch.float32), None if bias is None else bias.float()).to(x.dtype)
    assert torch.equal(ops.linear_mxfp4_ref(x, fw, bias), ref)
    out = torch.full((5, 1152), float("nan"), dtype=dtype) if with_out else None
    y = ops.linear(x, fw, bias, out)
    if with_out:
        assert y is out
    assert y.dtype == dtype and torch.equal(y, ref)


def test_dequant_op_cpu(quantised):
    _w, fw = quantised
    want = fw.dequant(torch.bfloat16)
    scratch = torch.full((1152 * 2048 + 64,), float("nan"), dtype=torch.bfloat16)
    got = ops.dequant_mxfp4(fw, scratch)
    assert got.data_ptr() == scratch.data_ptr() and torch.equal(got, want)
    assert torch.isnan(scratch[1152 * 2048:]).all()
    assert torch.equal(ops.dequant_mxfp4(fw), want)


def _engine(weight_quant=None, model=None, **kw):
    from dgi.engine import EngineConfig, LLMEngine
    from dgi.models.config import get_config
    return LLMEngine(EngineConfig(model="llama-tiny-hd128", device="cpu", dtype=torch.float32, num_blocks=256,
                                  max_num_seqs=8, max_model_len=512, max_num_batched_tokens=256, use_graphs=False,
                                  seed=3, weight_quant=weight_quant, **kw),
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

    qe = _engine("mxfp4")
    qm = qe.model
    assert qm.weight_quant == "mxfp4" and qm.act_quant is None and qm._quant_scratch is None   # CPU: no scratch
    expect = 0
    for L in qm.layers:
        for k in QUANT_SLOTS:
            fw = getattr(L, k)
            assert isinstance(fw, Mxfp4Weight)
            N, K = fw.shape
            expect += N * K // 2 + N * K // 32
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
            fw = quantize_mxfp4(w)
            assert torch.equal(fw.q, getattr(Lq, k).q) and torch.equal(fw.scale, getattr(Lq, k).scale)
            w.copy_(_decode(fw).float())

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
    e = _engine("mxfp4", model=m)
    assert e.model is m and m.weight_quant == "mxfp4"
    q0 = m.layers[0].qkv.q
    e2 = _engine("mxfp4", model=m)                # already quantised: left alone
    assert e2.model.layers[0].qkv.q is q0


def test_quantised_model_tensors_and_copy_from():
    from dgi.models.config import get_config
    from dgi.models.llama import LlamaModel
    mc = get_config("llama-tiny-hd128")
    m = LlamaModel(mc, "cpu", torch.float32, seed=3).quantize_weights("mxfp4")
    names = dict(m.tensors())
    assert names["layers.0.qkv.q"].dtype == torch.uint8 and names["layers.0.qkv.scale"].dtype == torch.uint8
    assert names["layers.0.qkv.scale"].shape == (m.layers[0].qkv.shape[0], m.layers[0].qkv.shape[1] // 32)
    assert "layers.0.qkv" not in names
    plain = LlamaModel(mc, "cpu", torch.float32, seed=4)
    with pytest.raises(RuntimeError, match="quantize_weights"):
        plain.copy_from(m)
    with pytest.raises(RuntimeError, match="quantize_weights"):
        m.copy_from(plain)
    with pytest.raises(RuntimeError, match="quantised"):
        m.fold_norms()
    with pytest.raises(RuntimeError, match="quantised"):
        m.load_state_dict_hf({})
    with pytest.raises(ValueError, match="'fp8', 'mxfp4'"):
        plain.quantize_weights("int8")
    with pytest.raises(ValueError, match="act_quant"):
        LlamaModel(mc, "cpu", torch.float32, seed=4).quantize_weights("mxfp4", act_quant="fp8")
    # a model in one mode is not re-quantised to the other, either way
    with pytest.raises(RuntimeError, match="mxfp4-quantised"):
        m.quantize_weights("fp8")
    f8 = LlamaModel(mc, "cpu", torch.float32, seed=4).quantize_weights("fp8")
    with pytest.raises(RuntimeError, match="fp8-quantised"):
        f8.quantize_weights("mxfp4")
    with pytest.raises(RuntimeError, match="quantize_weights"):
        f8.copy_from(m)
    assert isinstance(m.layers[0].qkv, Mxfp4Weight) and isinstance(f8.layers[0].qkv, ops.Fp8Weight)
    m2 = LlamaModel(mc, "cpu", torch.float32, seed=4).quantize_weights("mxfp4")
    assert not torch.equal(m2.layers[1].down.q, m.layers[1].down.q)
    m2.copy_from(m)
    assert torch.equal(m2.layers[1].down.q, m.layers[1].down.q)
    assert torch.equal(m2.layers[1].down.scale, m.layers[1].down.scale)


def test_pipeline_stage_model_serves_mxfp4():
    """A stage's partial model quantises like the whole model's layers of that range and runs the
    quantised layer loop (the pipeline engines call ``quantize_weights(cfg.weight_quant)`` on it)."""
    from dgi.models.config import get_config
    from dgi.models.llama import QUANT_SLOTS, LlamaModel
    mc = get_config("llama-tiny-hd128")
    whole = LlamaModel(mc, "cpu", torch.float32, seed=3).quantize_weights("mxfp4")
    n = len(whole.layers)
    assert n >= 2
    a, b = n // 2, n
    stage = LlamaModel(mc, "cpu", torch.float32, a, b, has_embed=False, has_head=True, seed=3)
    stage.quantize_weights("mxfp4")
    assert stage.weight_quant == "mxfp4" and len(stage.layers) == b - a
    names = dict(stage.tensors())
    assert f"layers.{a}.qkv.q" in names and "layers.0.qkv.q" not in names
    for L, Lw in zip(stage.layers, whole.layers[a:b]):
        for k in QUANT_SLOTS:
            assert torch.equal(getattr(L, k).q, getattr(Lw, k).q)
            assert torch.equal(getattr(L, k).scale, getattr(Lw, k).scale)
    # a one-stage engine over the stage's layer range runs them through _forward_layers_quant
    from dgi.engine import EngineConfig, LLMEngine
    from dgi.sched.request import SamplingParams
    e = LLMEngine(EngineConfig(model="llama-tiny-hd128", device="cpu", dtype=torch.float32, num_blocks=64,
                               max_num_seqs=4, max_model_len=256, max_num_batched_tokens=64, use_graphs=False,
                               enable_prefix_caching=False, seed=3, weight_quant="mxfp4"), model_cfg=mc)
    assert all(isinstance(getattr(L, k), Mxfp4Weight) for L in e.model.layers for k in QUANT_SLOTS)
    out = e.generate([[1, 5, 9]], SamplingParams(max_tokens=3, temperature=0.0, ignore_eos=True))
    assert len(out[0].output) == 3


def test_engine_config_modes():
    from dgi.engine import WEIGHT_QUANT_MODES, EngineConfig
    assert WEIGHT_QUANT_MODES == (None, "fp8", "mxfp4")
    with pytest.raises(ValueError, match="int4"):
        EngineConfig(weight_quant="int4")
    with pytest.raises(ValueError, match="weight_quant='fp8'"):
        EngineConfig(weight_quant="mxfp4", act_quant="fp8")
    cfg = EngineConfig(weight_quant="mxfp4", kv_dtype="fp8")
    # the pipeline and P/D engines copy the config field by field
    assert EngineConfig(**{**cfg.__dict__, "device": "cpu"}).weight_quant == "mxfp4"


def test_skinny_w4_cfg_table():
    assert set(ops.SKINNY_W4_CFGS) == set(range(1, 9))
    # a 4-wave config (the default among them) takes every K % 1024 == 0
    for K in (1024, 2048, 3072, 14336):
        assert ops.skinny_w4_cfg_ok(0, 96, K) and ops.skinny_w4_cfg_ok(1, 96, K) and ops.skinny_w4_cfg_ok(2, 96, K)
    assert ops.SKINNY_W4_CFGS[2][0] == 4
    assert {nw for nw, _nt, _u, _d in ops.SKINNY_W4_CFGS.values()} == {4, 8}
    assert {nt for _nw, nt, _u, _d in ops.SKINNY_W4_CFGS.values()} == {1, 2, 4}
    assert ops.skinny_w4_cfg_ok(3, 256, 14336) and ops.skinny_w4_cfg_ok(8, 256, 2048)
    assert not ops.skinny_w4_cfg_ok(3, 256, 1024)         # 8 waves: K % 2048
    assert not ops.skinny_w4_cfg_ok(5, 1168, 1024)        # two column tiles per wave: N % 32
    assert not ops.skinny_w4_cfg_ok(7, 96, 1024)          # four column tiles per wave: N % 64
    assert not ops.skinny_w4_cfg_ok(8, 256, 1024)
    assert not ops.skinny_w4_cfg_ok(1, 256, 3584)
    # whatever the picker chooses divides the shape
    for N, K in ((96, 1024), (1152, 2048), (6144, 4096), (28672, 4096), (4096, 14336), (10240, 8192), (57344, 8192)):
        for M in (1, 2, 3, 8, 9, 16, 17, 32):
            assert ops.skinny_w4_cfg_ok(ops._skinny_w4_cfg(M, N, K), N, K), (M, N, K)
            assert ops.skinny_w4_cfg_ok(ops._skinny_w4_cfg(M, N), N, K), (M, N, K)


@pytest.mark.parametrize("key,value,expect", [("quantization", "mxfp4", "mxfp4"), ("weight_quant", "MXFP4", "mxfp4"),
                                              ("quantization", "int4", None)])
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


def test_native_worker_act_quant_needs_fp8_weights(caplog):
    from engines.llm_native import NativeLLMEngine
    e = NativeLLMEngine({"model_id": "llama-tiny", "device": "cpu", "max_model_len": 256, "num_blocks": 64,
                         "max_num_seqs": 4, "quantization": "mxfp4", "act_quant": "fp8"})
    with caplog.at_level(logging.WARNING, logger="engines.llm_native"):
        e.load_model()
    try:
        assert (e.engine.cfg.weight_quant, e.engine.cfg.act_quant) == ("mxfp4", None)
        assert any("act_quant" in r.getMessage() for r in caplog.records)
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
        for argv, want in ((["--weight-quant", "mxfp4"], "mxfp4"), ([], None)):
            with pytest.raises(Stop):
                node.main(argv)
            assert seen["wq"] == want
        with pytest.raises(SystemExit):
            node.main(["--weight-quant", "int4"])
    finally:
        node.Router = orig
