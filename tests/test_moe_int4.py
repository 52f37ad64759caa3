"""INT4 weight-only experts of a Qwen3-MoE model (``expert_quant="awq"``) without a GPU: the container, the
reference on it, ``quantize_experts`` and the serving switches (the GPU side: tests/test_moe_int4_gpu.py)."""
import pytest
import torch

from dgi import ops

NAME = "qwen3-moe-tiny"


def test_container_equals_the_dense_quantiser_per_expert():
    w = torch.randn(3, 48, 256, generator=torch.Generator().manual_seed(0)) / 16
    iw = ops.quantize_int4_experts(w)
    assert iw.shape == w.shape and iw.device == w.device and iw.nbytes() == 4 * (3 * 48 * 32 + 3 * 48 * 2)
    for e in range(3):
        one = ops.quantize_int4(w[e])
        assert torch.equal(iw.q[e], one.q) and torch.equal(iw.sz[e], one.sz), e
        assert isinstance(iw[e], ops.Int4Weight) and iw[e].q.data_ptr() == iw.q[e].data_ptr()
        assert torch.equal(iw.dequant(torch.float32)[e], one.dequant(torch.float32))
    q, sz = iw.q, iw.sz
    for qq, ss in [(q.long(), sz), (q, sz.float()), (q[0], sz[0]), (q.transpose(0, 1), sz.transpose(0, 1)),
                   (q, sz[:, :, :1].contiguous()), (q, sz[:2]), (q[:, :, :24].contiguous(), sz)]:
        with pytest.raises(ValueError, match="Int4ExpertWeight"):
            ops.Int4ExpertWeight(qq, ss)
    with pytest.raises(ValueError):
        ops.quantize_int4_experts(w[0])


@pytest.mark.parametrize("E,k,H,I,T", [(8, 2, 512, 256, 64), (16, 4, 2048, 768, 48)])
def test_reference_takes_the_container(E, k, H, I, T):
    """``moe_mlp_ref`` on the containers is ``moe_mlp_ref`` on their dequantised copies, exactly; the relative rms
    against the unquantised experts is printed for profiles/moe_int4/README.md (no band is asserted on it)."""
    g = torch.Generator().manual_seed(E)
    router, x = torch.randn(E, H, generator=g) / H ** 0.5, torch.randn(T, H, generator=g)
    gate_up, down = torch.randn(E, 2 * I, H, generator=g) / H ** 0.5, torch.randn(E, H, I, generator=g) / I ** 0.5
    ids, _ = ops.moe_route_ref(x @ router.t(), k, True)
    qgu, qdn = ops.quantize_int4_experts(gate_up), ops.quantize_int4_experts(down)
    assert ops.moe_mlp_ok(x, router, qgu, qdn, k) is False          # CPU tensors: the reference
    got = ops.moe_mlp(x, router, qgu, qdn, k, True, ids=ids)
    assert torch.equal(got, ops.moe_mlp_ref(x, router, qgu.dequant(), qdn.dequant(), k, True, ids=ids))
    ref = ops.moe_mlp_ref(x, router, gate_up, down, k, True, ids=ids)
    print(f"E={E} H={H} I={I} T={T}: int4 relative rms {float((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()):.4f}")
    for a, b in ((qgu, down), (gate_up, qdn), (qgu, ops.quantize_fp8_experts(down))):     # a mixed pair raises
        with pytest.raises(ValueError, match="Int4ExpertWeight"):
            ops.moe_mlp(x, router, a, b, k, True)


def _model(name=NAME):
    from dgi.models.config import get_config
    from dgi.models.llama import LlamaModel
    return LlamaModel(get_config(name), "cpu", torch.float32, seed=3)


def test_quantize_experts_awq_model():
    m = _model()
    c, before = m.cfg, m.weight_bytes()
    assert m.quantize_experts("awq") is m and m.expert_quant == "int4" and m.weight_quant is None
    held = m.layers[0].experts_gate_up
    assert isinstance(held, ops.Int4ExpertWeight) and isinstance(m.layers[0].experts_down, ops.Int4ExpertWeight)
    assert held.shape == (c.num_experts, 2 * c.moe_intermediate_size, c.hidden_size)
    # an fp32 element (4 bytes) becomes half a byte of code and 4 bytes of scale / zero word per 128
    n = 3 * c.num_experts * c.moe_intermediate_size * c.hidden_size
    assert m.weight_bytes() == before - len(m.layers) * (4 * n - n // 2 - n // 32)
    assert m.quantize_experts("awq").layers[0].experts_gate_up is held          # a second call changes nothing
    for fn in (lambda: m.copy_from(_model()), lambda: _model().copy_from(m), lambda: m.load_state_dict_hf({}),
               m.fold_norms, lambda: m.quantize_experts("fp8")):
        with pytest.raises(RuntimeError, match="quantize_experts"):
            fn()
    with pytest.raises(ValueError, match="dense"):
        _model("llama-tiny-hd128").quantize_experts("awq")


def test_switches(monkeypatch):
    from dgi.engine import EngineConfig, LLMEngine, refuse_expert_quant
    from dgi.serve import node
    from engines.llm_native import NativeLLMEngine
    cfg = EngineConfig(model=NAME, device="cpu", dtype=torch.float32, num_blocks=64, max_num_seqs=4, max_model_len=256,
                       max_num_batched_tokens=256, use_graphs=False, expert_quant="awq")
    m = _model().quantize_experts("awq")
    held = m.layers[0].experts_down
    assert LLMEngine(cfg, model_cfg=m.cfg, model=m).model.layers[0].experts_down is held     # quantised before: left alone
    assert isinstance(LLMEngine(cfg, model_cfg=m.cfg).model.layers[1].experts_gate_up, ops.Int4ExpertWeight)
    with pytest.raises(ValueError, match="expert_quant='awq' is not supported with tensor parallel"):
        refuse_expert_quant(cfg, "tensor parallel")
    w = NativeLLMEngine({"model_id": NAME, "device": "cpu", "max_model_len": 256, "num_blocks": 64, "max_num_seqs": 4,
                         "expert_quant": "AWQ"})
    w.load_model()
    try:
        assert w.engine.cfg.expert_quant == "awq" and w.engine.model.expert_quant == "int4"
    finally:
        w.unload_model()
    seen = []
    monkeypatch.setattr(node, "Router", lambda args, fabric, layout: seen.append(args.expert_quant) or 1 / 0)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(ZeroDivisionError):
        node.main(["--expert-quant", "awq"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):                                  # a multi-rank run is refused before set-up
        node.main(["--expert-quant", "awq"])
    assert seen == ["awq"]
