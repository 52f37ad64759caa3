"""FP8 weight-only experts of a Qwen3-MoE model (``expert_quant="fp8"``) without a GPU: the
``Fp8ExpertWeight`` container and its quantiser, the quantisation error of the block, the model's
``quantize_experts``, the engine and the serving surfaces (the GPU side: tests/test_moe_fp8_gpu.py)."""
import logging

import pytest
import torch

from dgi import ops

NAME = "qwen3-moe-tiny"


# ---------------------------------------------------------------------------- container and quantiser

def _experts_with_edge_rows():
    g = torch.Generator().manual_seed(0)
    w = torch.randn(5, 48, 256, generator=g) / 16
    w[1, 7] = 0.0                    # an all-zero row: scale 1, codes 0
    w[3, 11, 100] = 1e4              # an outlier: the rest of its row underflows towards 0
    return w


def test_quantiser_equals_the_dense_one_per_expert():
    w = _experts_with_edge_rows()
    fw = ops.quantize_fp8_experts(w)
    assert isinstance(fw, ops.Fp8ExpertWeight)
    assert fw.q.dtype == torch.float8_e4m3fn and fw.q.shape == (5, 48, 256) and fw.q.is_contiguous()
    assert fw.scale.dtype == torch.float32 and fw.scale.shape == (5, 48) and fw.scale.is_contiguous()
    assert fw.shape == w.shape and fw.device == w.device
    assert fw.nbytes() == 5 * 48 * 256 + 4 * 5 * 48
    full = fw.dequant(torch.float32)
    assert full.shape == w.shape and full.dtype == torch.float32
    for e in range(5):
        one = ops.quantize_fp8(w[e])
        assert torch.equal(fw.q[e].view(torch.uint8), one.q.view(torch.uint8)), e
        assert torch.equal(fw.scale[e], one.scale), e
        view = fw[e]
        assert isinstance(view, ops.Fp8Weight) and view.shape == (48, 256)
        assert view.q.data_ptr() == fw.q[e].data_ptr() and view.scale.data_ptr() == fw.scale[e].data_ptr()
        assert torch.equal(view.dequant(torch.float32), one.dequant(torch.float32))
        assert torch.equal(full[e], one.q.float() * one.scale[:, None])
    assert float(fw.scale[1, 7]) == 1.0 and not fw.q[1, 7].float().any()
    assert float(fw.q[3, 11, 100].float()) == 448.0 and torch.isfinite(full).all()
    assert torch.equal(fw.dequant(torch.bfloat16), full.bfloat16())
    # bf16 in: the same codes as the dense quantiser gives on the bf16 rows
    fb = ops.quantize_fp8_experts(w.bfloat16())
    assert torch.equal(fb.q[2].view(torch.uint8), ops.quantize_fp8(w[2].bfloat16()).q.view(torch.uint8))
    with pytest.raises(ValueError):
        ops.quantize_fp8_experts(w[0])


def test_constructor_refusals():
    q = torch.zeros(3, 16, 32).to(torch.float8_e4m3fn)
    s = torch.ones(3, 16)
    ops.Fp8ExpertWeight(q, s)
    bad = [(q.view(torch.uint8), s),                                   # dtype of the codes
           (torch.zeros(3, 16, 32, dtype=torch.bfloat16), s),
           (q, s.double()),                                            # dtype of the scales
           (q[0], s[0]),                                               # rank
           (q.view(3, 16, 2, 16), s),
           (torch.zeros(3, 32, 16).to(torch.float8_e4m3fn).transpose(1, 2), s),      # contiguity
           (q, torch.ones(16, 3).t()),
           (q, torch.ones(3, 32)),                                     # scale shape
           (q, torch.ones(3)),
           (q, torch.ones(3, 16, 1))]
    for qq, ss in bad:
        with pytest.raises(ValueError, match="Fp8ExpertWeight"):
            ops.Fp8ExpertWeight(qq, ss)


# ---------------------------------------------------------------------------- quantisation error of the block

@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("E,k,H,I,T", [(8, 2, 512, 256, 64), (16, 4, 2048, 768, 48)])
def test_block_quantisation_error(E, k, H, I, T, seed):
    """``moe_mlp_ref`` over quantised experts against the fp32 weights, the routing forced to the same
    ids: per-channel e4m3 (3 mantissa bits) through two projections.  0.0457-0.0466 relative rms was
    measured on these six cases; the upper bound is 1.3x that, the lower bound proves the weights
    really were quantised."""
    g = torch.Generator().manual_seed(seed)
    router = torch.randn(E, H, generator=g) / H ** 0.5
    gate_up = torch.randn(E, 2 * I, H, generator=g) / H ** 0.5
    down = torch.randn(E, H, I, generator=g) / I ** 0.5
    x = torch.randn(T, H, generator=g)
    ids, _ = ops.moe_route_ref(x @ router.t(), k, True)
    ref = ops.moe_mlp_ref(x, router, gate_up, down, k, True, ids=ids)
    qgu, qdn = ops.quantize_fp8_experts(gate_up), ops.quantize_fp8_experts(down)
    assert ops.moe_mlp_ok(x, router, qgu, qdn, k) is False          # a CPU tensor: the reference
    got = ops.moe_mlp(x, router, qgu, qdn, k, True, ids=ids)
    assert torch.equal(got, ops.moe_mlp_ref(x, router, qgu, qdn, k, True, ids=ids))
    # the container is its dequantised copy
    assert torch.equal(got, ops.moe_mlp_ref(x, router, qgu.dequant(), qdn.dequant(), k, True, ids=ids))
    rel = float((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
    print(f"E={E} k={k} H={H} I={I} T={T} seed={seed}: relative rms {rel:.4f}")
    assert 0.02 < rel < 0.06, rel
    for a, b in ((qgu, down), (gate_up, qdn)):                      # a mixed pair raises
        for fn in (ops.moe_mlp, ops.moe_mlp_ref):
            with pytest.raises(ValueError, match="Fp8ExpertWeight"):
                fn(x, router, a, b, k, True)
        with pytest.raises(ValueError, match="Fp8ExpertWeight"):
            ops.moe_mlp_ok(x, router, a, b, k)


def test_moe_gemm_ref_takes_the_container():
    g = torch.Generator().manual_seed(3)
    E, k, T, K, N, BM = 4, 2, 9, 64, 32, 16
    ids = torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(T)]).to(torch.int32)
    _c, _o, sorted_slot, block_expert, _inv = ops.moe_align(ids, E, BM)
    x = torch.randn(T, K, generator=g)
    fw = ops.quantize_fp8_experts(torch.randn(E, 2 * N, K, generator=g) / 8)
    for epi in (ops.MOE_EPI_SWIGLU,):
        got = ops.moe_gemm(x, fw, sorted_slot, block_expert, k, epi, BM)
        assert got.shape == (sorted_slot.numel(), N)
        assert torch.equal(got, ops.moe_gemm_ref(x, fw.dequant(), sorted_slot, block_expert, k, epi, BM))


# ---------------------------------------------------------------------------- model

def _model(seed=3, name=NAME):
    from dgi.models.config import get_config
    from dgi.models.llama import LlamaModel
    return LlamaModel(get_config(name), "cpu", torch.float32, seed=seed)


def test_quantize_experts_model():
    from dgi.models.llama import EXPERT_SLOTS
    m = _model()
    c = m.cfg
    E, Im, H = c.num_experts, c.moe_intermediate_size, c.hidden_size
    keep = {n: t.clone() for n, t in m.tensors() if "experts_" not in n}
    assert any(n.endswith(".router") for n in keep) and any(n.endswith(".qkv") for n in keep) and "embed" in keep
    experts = {(i, k): getattr(L, k).clone() for i, L in enumerate(m.layers) for k in EXPERT_SLOTS}
    before = m.weight_bytes()
    assert m.expert_quant is None
    assert m.quantize_experts("fp8") is m and m.expert_quant == "fp8" and m.weight_quant is None
    held = [m.layers[0].experts_gate_up, m.layers[0].experts_down.q]
    m.quantize_experts("fp8")                                       # idempotent
    assert m.layers[0].experts_gate_up is held[0] and m.layers[0].experts_down.q is held[1]
    # codes + scales, exact: E*N*K + 4*E*N per tensor, instead of 4 bytes per fp32 element
    per_layer_fp32 = 4 * (E * 2 * Im * H + E * H * Im)
    per_layer_fp8 = (E * 2 * Im * H + 4 * E * 2 * Im) + (E * H * Im + 4 * E * H)
    assert m.weight_bytes() == before - len(m.layers) * (per_layer_fp32 - per_layer_fp8)
    for (i, k), w in experts.items():
        fw = getattr(m.layers[i], k)
        assert isinstance(fw, ops.Fp8ExpertWeight) and fw.shape == w.shape
        for e in (0, E - 1):
            one = ops.quantize_fp8(w[e])
            assert torch.equal(fw.q[e].view(torch.uint8), one.q.view(torch.uint8)) and torch.equal(fw.scale[e], one.scale)
    # qkv, o, the router, the norms and the embeddings: bit-unchanged
    now = dict(m.tensors())
    for n, t in keep.items():
        assert torch.equal(now[n], t) and now[n].dtype == t.dtype, n
    names = [n for n, _ in m.tensors()]
    for k in EXPERT_SLOTS:
        assert f"layers.0.{k}.q" in names and f"layers.0.{k}.scale" in names and f"layers.0.{k}" not in names

    # copy_from round-trips codes and scales into a model quantised from other weights
    other = _model(seed=9).quantize_experts("fp8")
    assert not torch.equal(other.layers[0].experts_down.scale, m.layers[0].experts_down.scale)
    other.copy_from(m)
    for (n, a), (n2, b) in zip(other.tensors(), m.tensors()):
        assert n == n2
        assert torch.equal(a.view(torch.uint8) if a.dtype == torch.float8_e4m3fn else a,
                           b.view(torch.uint8) if b.dtype == torch.float8_e4m3fn else b), n
    plain = _model(seed=9)
    with pytest.raises(RuntimeError, match="quantize_experts"):
        plain.copy_from(m)
    with pytest.raises(RuntimeError, match="quantize_experts"):
        m.copy_from(plain)
    # writers of the expert tensors refuse a quantised model
    with pytest.raises(RuntimeError, match="quantize_experts"):
        m.load_state_dict_hf({})
    with pytest.raises(RuntimeError, match="quantize_experts"):
        m.fold_norms()


def test_quantize_experts_refusals():
    m = _model()
    with pytest.raises(ValueError, match="mxfp4.*not supported for experts yet"):
        m.quantize_experts("mxfp4")
    with pytest.raises(ValueError, match="int4"):
        m.quantize_experts("int4")
    assert m.expert_quant is None and isinstance(m.layers[0].experts_down, torch.Tensor)
    with pytest.raises(ValueError, match="dense"):
        _model(name="llama-tiny-hd128").quantize_experts("fp8")
    # the projections of a MoE model stay as they are, before and after
    for mm in (m, _model().quantize_experts("fp8")):
        for mode in ("fp8", "mxfp4"):
            with pytest.raises(ValueError, match="MoE.*quantize_experts"):
                mm.quantize_weights(mode)


# ---------------------------------------------------------------------------- engine and surfaces

def _engine(name=NAME, model=None, **kw):
    from dgi.engine import EngineConfig, LLMEngine
    from dgi.models.config import get_config
    return LLMEngine(EngineConfig(model=name, device="cpu", dtype=torch.float32, num_blocks=256, max_num_seqs=8,
                                  max_model_len=512, max_num_batched_tokens=256, use_graphs=False, seed=3, **kw),
                     model_cfg=get_config(name), model=model)


def test_engine_config_field():
    from dgi.engine import EngineConfig
    with pytest.raises(ValueError, match="int4"):
        EngineConfig(expert_quant="int4")
    with pytest.raises(ValueError, match="expert_quant"):
        EngineConfig(expert_quant="mxfp4")
    assert EngineConfig().expert_quant is None
    cfg = EngineConfig(expert_quant="fp8", kv_dtype="fp8")
    assert EngineConfig(**{**cfg.__dict__, "device": "cpu"}).expert_quant == "fp8"
    # the multi-rank layouts refuse the knob at configuration time
    from dgi.engine import refuse_expert_quant
    refuse_expert_quant(EngineConfig(), "the layer pipeline")
    with pytest.raises(ValueError, match="expert_quant='fp8' is not supported with the layer pipeline"):
        refuse_expert_quant(cfg, "the layer pipeline")
    with pytest.raises(ValueError, match="dense"):
        _engine("llama-tiny-hd128", expert_quant="fp8")
    with pytest.raises(ValueError, match="MoE.*expert_quant"):
        _engine(weight_quant="fp8")


def test_cpu_engine_generates_with_quantised_experts():
    from dgi.models.llama import EXPERT_SLOTS
    from dgi.sched.request import SamplingParams
    sp = SamplingParams(max_tokens=8, temperature=0.0, ignore_eos=True)
    prompts = [[1, 5, 9, 13, 17, 21, 25, 29] * 3, [1, 2, 3]]
    qe = _engine(expert_quant="fp8")
    assert qe.model.expert_quant == "fp8" and isinstance(qe.model.layers[0].experts_gate_up, ops.Fp8ExpertWeight)
    out = [r.output for r in qe.generate(prompts, sp)]
    assert all(len(o) == 8 for o in out)
    # an engine handed a model that was quantised beforehand leaves it alone
    m = _model().quantize_experts("fp8")
    held = m.layers[0].experts_gate_up
    pe = _engine(model=m, expert_quant="fp8")
    assert pe.model is m and m.layers[0].experts_gate_up is held
    assert [r.output for r in pe.generate(prompts, sp)] == out
    # and one handed the bf16-free model quantises it
    m2 = _model()
    assert _engine(model=m2, expert_quant="fp8").model.expert_quant == "fp8"
    # the same fp32 math over the dequantised copies: token equality
    plain = _engine()
    assert plain.model.expert_quant is None and plain.model.weight_bytes() > qe.model.weight_bytes()
    for L, Lq in zip(plain.model.layers, qe.model.layers):
        for k in EXPERT_SLOTS:
            getattr(L, k).copy_(getattr(Lq, k).dequant(torch.float32))
    assert [r.output for r in plain.generate(prompts, sp)] == out


@pytest.mark.parametrize("model_id,value,expect", [(NAME, "fp8", "fp8"), (NAME, "FP8", "fp8"), (NAME, "none", None),
                                                   (NAME, "int4", None), ("llama-tiny", "fp8", None)])
def test_native_worker_expert_quant_key(model_id, value, expect, caplog):
    from engines.llm_native import NativeLLMEngine
    e = NativeLLMEngine({"model_id": model_id, "device": "cpu", "max_model_len": 256, "num_blocks": 64,
                         "max_num_seqs": 4, "expert_quant": value})
    with caplog.at_level(logging.WARNING, logger="engines.llm_native"):
        e.load_model()
    try:
        assert e.engine.model.expert_quant == expect and e.engine.cfg.expert_quant == expect
        warned = [r for r in caplog.records if "expert_quant" in r.getMessage() and "fp8" in r.getMessage()]
        assert bool(warned) == (expect is None and value != "none")
    finally:
        e.unload_model()


def test_node_parses_expert_quant(monkeypatch):
    from dgi.serve import node
    seen = {}

    class Stop(Exception):
        pass

    def fake_router(args, fabric, layout):
        seen["eq"] = args.expert_quant
        raise Stop
    monkeypatch.setattr(node, "Router", fake_router)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for argv, want in ((["--expert-quant", "fp8"], "fp8"), ([], None)):
        with pytest.raises(Stop):
            node.main(argv)
        assert seen["eq"] == want
    with pytest.raises(SystemExit):
        node.main(["--expert-quant", "int4"])
    # the multi-rank layouts refuse it before anything is set up
    monkeypatch.setenv("WORLD_SIZE", "2")
    seen.clear()
    with pytest.raises(SystemExit):
        node.main(["--expert-quant", "fp8"])
    assert not seen
