"""Qwen3-MoE on the CPU: config translation, the torch definitions of the MoE ops, Hugging Face
parity in fp32, pipeline splits and the refusals."""
import hashlib
import math

import pytest
import torch

from dgi import ops
from dgi.models.config import ModelConfig, PRESETS, get_config
from dgi.models.llama import LlamaModel

H, IM, L, NH, NKV, HD, V, E, K = 512, 256, 2, 8, 2, 128, 1024, 8, 2       # qwen3-moe-tiny's geometry
HF_PROMPTS = [[1, 33, 44, 55, 66, 77, 88, 99, 111, 222], [1] + list(range(300, 300 + 139))]     # 10 and 140 tokens


# ---------------------------------------------------------------------------- config

def _hf_dict(**over):
    d = {"model_type": "qwen3_moe", "vocab_size": V, "hidden_size": H, "intermediate_size": 1024,
         "moe_intermediate_size": IM, "num_hidden_layers": L, "num_attention_heads": NH, "num_key_value_heads": NKV,
         "head_dim": HD, "num_experts": E, "num_experts_per_tok": K, "norm_topk_prob": True, "decoder_sparse_step": 1,
         "mlp_only_layers": [], "max_position_embeddings": 1024, "rms_norm_eps": 1e-6, "bos_token_id": 1,
         "eos_token_id": 2, "tie_word_embeddings": False, "rope_theta": 1000000.0}
    d.update(over)
    return {k: v for k, v in d.items() if v is not None}


@pytest.mark.parametrize("key", ["num_experts", "num_local_experts"])
def test_config_translation_reads_either_expert_count(key):
    mc = ModelConfig.from_hf_dict(_hf_dict(**{"num_experts": None, key: E}), name="x")
    assert mc.arch == "qwen3_moe" and mc.qk_norm and mc.is_moe
    assert (mc.num_experts, mc.num_experts_per_tok, mc.moe_intermediate_size, mc.norm_topk_prob) == (E, K, IM, True)
    assert mc.head_dim == HD and mc.num_kv_heads == NKV and mc.rope_theta == 1e6


@pytest.mark.parametrize("over", [{"decoder_sparse_step": 2}, {"mlp_only_layers": [0]}, {"use_sliding_window": True},
                                  {"layer_types": ["full_attention", "sliding_attention"]}])
def test_unsupported_settings_raise(over):
    with pytest.raises(ValueError):
        ModelConfig.from_hf_dict(_hf_dict(**over), name="x")


def test_dense_configs_are_dense():
    assert not get_config("qwen3-tiny").is_moe and not get_config("llama3-8b").is_moe


def test_presets():
    c = get_config("qwen3-30b-a3b")
    assert (c.arch, c.num_layers, c.hidden_size, c.num_heads, c.num_kv_heads, c.head_dim) == \
        ("qwen3_moe", 48, 2048, 32, 4, 128)
    assert (c.num_experts, c.num_experts_per_tok, c.moe_intermediate_size, c.norm_topk_prob) == (128, 8, 768, True)
    assert (c.vocab_size, c.rope_theta, c.rms_eps, c.qk_norm) == (151936, 1e6, 1e-6, True)
    assert 30.0e9 < c.param_count() < 31.0e9
    t = get_config("qwen3-moe-tiny")
    assert (t.num_layers, t.hidden_size, t.num_heads, t.num_kv_heads, t.head_dim, t.vocab_size) == \
        (L, H, NH, NKV, HD, V)
    assert (t.num_experts, t.num_experts_per_tok, t.moe_intermediate_size, t.qk_norm) == (E, K, IM, True)
    assert get_config("qwen3-30b-a3b@L8").num_layers == 8


@pytest.mark.parametrize("name", ["Qwen/Qwen3-30B-A3B", "Qwen/Qwen3-235B-A22B"])
def test_hub_names_still_raise(name):
    with pytest.raises(KeyError) as ei:
        get_config(name)
    if "30B" in name:
        assert "qwen3-30b-a3b" in str(ei.value)      # the message names the preset


def test_param_count_is_the_tensor_total():
    c = get_config("qwen3-moe-tiny")
    m = LlamaModel(c, "cpu", seed=1)
    assert sum(t.numel() for _, t in m.tensors()) == c.param_count()
    assert m.weight_bytes() == 2 * c.param_count()
    Lw = m.layers[0]
    assert Lw.gate_up is None and Lw.down is None
    assert tuple(Lw.router.shape) == (E, H) and tuple(Lw.experts_gate_up.shape) == (E, 2 * IM, H)
    assert tuple(Lw.experts_down.shape) == (E, H, IM)


def _weights_sha256(name, seed):
    m = LlamaModel(get_config(name), "cpu", seed=seed)
    h = hashlib.sha256()
    for n, t in m.tensors():
        h.update(n.encode())
        h.update(t.contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


# recorded with this function on the commit before the experts were added (seed 0, CPU, bf16)
PARENT_SHA256 = {"qwen3-tiny": "a42302a01ca3f72a2f42aa67f8b5fda40e2d0864304b61a5cc9c4fe332aed4e8",
                 "llama-tiny": "cdd8f6a840c29a4b4c4450cec28545e1d4bff4fa2087bfd0257ae8769d05f3dd"}


@pytest.mark.parametrize("name", sorted(PARENT_SHA256))
def test_dense_models_keep_their_random_weights(name):
    assert _weights_sha256(name, 0) == PARENT_SHA256[name]


def test_copy_from_carries_the_experts():
    c = get_config("qwen3-moe-tiny")
    src = LlamaModel(c, "cpu", seed=3)
    dst = LlamaModel(c, "cpu", torch.float32, init="empty").copy_from(src)
    for a, b in zip(src.layers, dst.layers):
        for k in ("router", "experts_gate_up", "experts_down"):
            assert torch.equal(getattr(a, k).float(), getattr(b, k))


# ---------------------------------------------------------------------------- the _ref definitions

def test_route_ref_tie_rule_and_both_normalisations():
    # experts 1, 4 and 6 tie for the maximum, expert 2 follows: k = 3 takes 1, 4, 6 in index order
    logits = torch.tensor([[0.5, 2.0, 1.5, -1.0, 2.0, 0.0, 2.0, 1.0]])
    lf = [float(v) for v in logits[0].double()]
    ex = [math.exp(v - max(lf)) for v in lf]
    for k, want in ((3, [1, 4, 6]), (4, [1, 4, 6, 2]), (1, [1])):
        for norm in (True, False):
            ids, w = ops.moe_route_ref(logits, k, norm)
            assert ids.dtype == torch.int32 and w.dtype == torch.float32
            assert ids[0].tolist() == want
            den = sum(ex[i] for i in want) if norm else sum(ex)
            ref = torch.tensor([ex[i] / den for i in want], dtype=torch.float64)
            torch.testing.assert_close(w[0].double(), ref, atol=1e-6, rtol=1e-6)
            if norm:
                assert abs(float(w.sum()) - 1.0) < 1e-6
    # selection is on the logits: two logits one ulp apart share an fp32 probability far from the maximum
    a = torch.tensor([[10.0, -20.0, float(torch.nextafter(torch.tensor(-20.0), torch.tensor(0.0))), -30.0]])
    ids, _ = ops.moe_route_ref(a, 2, True)
    assert ids[0].tolist() == [0, 2]
    assert ops.moe_route(a, 2, True)[0][0].tolist() == [0, 2]        # the CPU op is the definition


def test_align_ref_layout():
    ids = torch.tensor([[3, 0], [3, 5], [0, 3], [5, 3]], dtype=torch.int32)
    counts, offsets, sorted_slot, block_expert, inv = ops.moe_align_ref(ids, 6, 16)
    assert counts.tolist() == [2, 0, 0, 4, 0, 2]
    assert offsets.tolist() == [0, 16, 16, 16, 32, 32, 48]
    P = ops.moe_capacity(8, 6, 16)
    assert P == 16 * (1 + 6) and sorted_slot.numel() == P and block_expert.numel() == P // 16
    assert sorted_slot[:2].tolist() == [1, 4] and sorted_slot[16:20].tolist() == [0, 2, 5, 7]
    assert sorted_slot[32:34].tolist() == [3, 6]
    assert int((sorted_slot >= 0).sum()) == 8
    assert block_expert.tolist() == [0, 3, 5, -1, -1, -1, -1]
    assert all(int(sorted_slot[int(inv[s])]) == s for s in range(8))


def test_gemm_and_combine_refs_against_fp64():
    g = torch.Generator().manual_seed(0)
    T, k, Ei, Hh, Ii = 5, 2, 4, 32, 16
    x = torch.randn(T, Hh, generator=g).bfloat16()
    gu = (0.2 * torch.randn(Ei, 2 * Ii, Hh, generator=g)).bfloat16()
    dn = (0.2 * torch.randn(Ei, Hh, Ii, generator=g)).bfloat16()
    ids = torch.tensor([[0, 3], [3, 1], [1, 0], [3, 0], [2, 3]], dtype=torch.int32)
    w = torch.tensor([[0.75, 0.25], [0.5, 0.5], [0.9, 0.1], [0.6, 0.4], [0.3, 0.7]])
    _c, _o, ss, be, inv = ops.moe_align_ref(ids, Ei, 16)
    act = ops.moe_gemm_ref(x, gu, ss, be, k, ops.MOE_EPI_SWIGLU, 16)
    y = ops.moe_gemm_ref(act, dn, ss, be, k, ops.MOE_EPI_PLAIN, 16)
    out = ops.moe_combine_ref(y, inv, w)
    for t in range(T):
        acc = torch.zeros(Hh, dtype=torch.float32)
        for j in range(k):
            e = int(ids[t, j])
            gate_up = x[t].double() @ gu[e].double().t()
            a = (torch.nn.functional.silu(gate_up[:Ii]) * gate_up[Ii:]).bfloat16()
            assert torch.equal(a, act[int(inv[t * k + j])])           # fp32 vs fp64 sums round alike here
            yy = (a.double() @ dn[e].double().t()).bfloat16()
            # combine order: products rounded to fp32, added in j order, one rounding at the end
            acc = acc + (w[t, j] * yy.float())
        assert torch.equal(out[t], acc.bfloat16()), t
    # a slot whose row is -1 contributes nothing
    inv2 = inv.clone()
    inv2[1] = -1
    out2 = ops.moe_combine_ref(y, inv2, w)
    assert torch.equal(out2[0], (w[0, 0] * y[int(inv[0])].float()).bfloat16())


def test_moe_mlp_ref_is_the_composition_and_forced_ids_use_the_models_probabilities():
    g = torch.Generator().manual_seed(1)
    T = 9
    x = torch.randn(T, H, generator=g)
    rw = 0.1 * torch.randn(E, H, generator=g)
    gu = 0.05 * torch.randn(E, 2 * IM, H, generator=g)
    dn = 0.05 * torch.randn(E, H, IM, generator=g)
    out = ops.moe_mlp(x, rw, gu, dn, K, True)
    logits = x @ rw.t()
    ids, w = ops.moe_route_ref(logits, K, True)
    _c, _o, ss, be, inv = ops.moe_align_ref(ids, E, 16)
    y = ops.moe_gemm_ref(ops.moe_gemm_ref(x, gu, ss, be, K, 1, 16), dn, ss, be, K, 0, 16)
    torch.testing.assert_close(out, ops.moe_combine_ref(y, inv, w), atol=1e-5, rtol=1e-5)
    forced = torch.flip(ids, dims=[1])
    out_f = ops.moe_mlp(x, rw, gu, dn, K, True, ids=forced)
    torch.testing.assert_close(out_f, out, atol=1e-5, rtol=1e-5)      # same experts, same renormalised weights
    other = (ids + 1) % E
    assert not torch.allclose(ops.moe_mlp(x, rw, gu, dn, K, True, ids=other), out, atol=1e-3)


# ---------------------------------------------------------------------------- HF parity (fp32)

def hf_moe_model(seed):
    """A local Qwen3MoeForCausalLM of qwen3-moe-tiny's geometry, initialised as tests/test_qwen3_gpu.py
    initialises its HF model (std 0.04, gains 1 +- 0.1)."""
    transformers = pytest.importorskip("transformers")
    cfg = transformers.Qwen3MoeConfig(vocab_size=V, hidden_size=H, intermediate_size=1024, moe_intermediate_size=IM,
                                      num_hidden_layers=L, num_attention_heads=NH, num_key_value_heads=NKV,
                                      head_dim=HD, num_experts=E, num_experts_per_tok=K, norm_topk_prob=True,
                                      decoder_sparse_step=1, mlp_only_layers=[], max_position_embeddings=1024,
                                      rms_norm_eps=1e-6, bos_token_id=1, eos_token_id=2, tie_word_embeddings=False,
                                      rope_theta=1000000.0)
    model = transformers.Qwen3MoeForCausalLM(cfg)
    torch.manual_seed(seed)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "norm" in n:
                p.copy_(1.0 + 0.1 * torch.randn_like(p))
            else:
                p.normal_(0.0, 0.04)
    return model.eval().float()


def hf_min_routing_gap(model, token_lists):
    """HF's own smallest gap between the k-th and (k+1)-th routing probability over these inputs."""
    gaps = []

    def hook(_m, _inp, out):
        p = torch.softmax(out[0].float(), dim=-1).sort(dim=-1, descending=True).values
        gaps.append(float((p[:, K - 1] - p[:, K]).min()))
    hs = [layer.mlp.gate.register_forward_hook(hook) for layer in model.model.layers]
    with torch.no_grad():
        outs = [model(torch.tensor([t])).logits[0] for t in token_lists]
    for h in hs:
        h.remove()
    return min(gaps), outs


@pytest.mark.parametrize("seed", [0, 1])
def test_per_position_logits_match_hf(tmp_path, seed):
    from dgi.engine import EngineConfig, LLMEngine
    from dgi.sched.request import SamplingParams
    model = hf_moe_model(seed)
    model.save_pretrained(str(tmp_path), safe_serialization=True)
    eng = LLMEngine(EngineConfig(model_path=str(tmp_path), device="cpu", dtype=torch.float32, num_blocks=64,
                                 max_num_seqs=4, max_model_len=512, max_num_batched_tokens=256, use_graphs=False,
                                 enable_prefix_caching=False))
    mc = eng.model.cfg
    assert mc.arch == "qwen3_moe" and mc.num_experts == E and mc.qk_norm and mc.norm_topk_prob
    steps = []
    orig = eng.model.compute_logits

    def spy(h, residual, idx):
        out = orig(h, residual, idx)
        steps.append(out.detach().float())
        return out
    eng.model.compute_logits = spy
    n_new = 12
    sp = SamplingParams(max_tokens=n_new, temperature=0.0, ignore_eos=True)
    runs = []
    for prompt in HF_PROMPTS:
        steps.clear()
        toks = eng.generate([prompt], sp)[0].output
        assert len(steps) == n_new
        runs.append((prompt, toks, [s[-1].clone() for s in steps]))
    gap, refs = hf_min_routing_gap(model, [p + t for p, t, _ in runs])
    print(f"seed {seed}: HF's smallest routing gap {gap:.3e}")
    assert gap > 1e-5, gap          # a condition on the inputs: no routing decision is a coin toss
    worst = 0.0
    for (prompt, toks, got), ref in zip(runs, refs):
        for t in range(n_new):
            err = float((got[t] - ref[len(prompt) - 1 + t]).abs().max())
            worst = max(worst, err)
            assert err <= 1e-4, (len(prompt), t, err)
    print(f"seed {seed}: worst |native - hf| logit {worst:.3e}")
    # the same weights through load_state_dict_hf (transformers' fused in-memory expert tensors)
    sd = model.state_dict()
    assert "model.layers.0.mlp.experts.gate_up_proj" in sd
    m2 = LlamaModel(mc, "cpu", torch.float32, init="empty")
    m2.load_state_dict_hf(sd)
    a, b = dict(eng.model.tensors()), dict(m2.tensors())
    assert a.keys() == b.keys()
    for name in a:
        assert torch.equal(a[name], b[name]), name


def test_missing_expert_tensor_is_a_keyerror_that_names_it(tmp_path):
    from safetensors.torch import save_file
    model = hf_moe_model(0)
    sd = model.state_dict()
    mc = ModelConfig.from_hf_dict(model.config.to_dict(), name="hf")
    per_expert = {}
    for k, v in sd.items():
        if k.endswith("experts.gate_up_proj"):
            for e in range(E):
                per_expert[k.replace("gate_up_proj", f"{e}.gate_proj.weight")] = v[e, :IM].clone()
                per_expert[k.replace("gate_up_proj", f"{e}.up_proj.weight")] = v[e, IM:].clone()
        elif k.endswith("experts.down_proj"):
            for e in range(E):
                per_expert[k.replace("down_proj", f"{e}.down_proj.weight")] = v[e].clone()
        else:
            per_expert[k] = v.clone()
    # the per-expert names load through load_state_dict_hf as well
    m = LlamaModel(mc, "cpu", torch.float32, init="empty")
    m.load_state_dict_hf(per_expert)
    assert torch.equal(m.layers[1].experts_gate_up, sd["model.layers.1.mlp.experts.gate_up_proj"])
    gone = "model.layers.1.mlp.experts.5.up_proj.weight"
    broken = {k: v for k, v in per_expert.items() if k != gone}
    with pytest.raises(KeyError, match="experts.5.up_proj"):
        LlamaModel(mc, "cpu", torch.float32, init="empty").load_state_dict_hf(broken)
    save_file(broken, str(tmp_path / "model.safetensors"))
    with pytest.raises(KeyError, match="experts.5.up_proj"):
        LlamaModel(mc, "cpu", torch.float32, checkpoint=str(tmp_path))


# ---------------------------------------------------------------------------- pipeline split, hook, refusals

def test_layer_ranges_equal_the_whole_model():
    """Layers [0, 1) + [1, 2) of qwen3-moe-tiny, fed every step of the whole model's engine, produce its
    logits bit for bit on the CPU (a layer's weights do not depend on the layer range, and the
    stream between two stages is the one the fused add would have made)."""
    from dgi.engine import EngineConfig, LLMEngine
    from dgi.sched.request import SamplingParams
    c = get_config("qwen3-moe-tiny")
    whole = LlamaModel(c, "cpu", seed=4)
    a = LlamaModel(c, "cpu", seed=4, layer_start=0, layer_end=1)
    b = LlamaModel(c, "cpu", seed=4, layer_start=1, layer_end=2)
    assert a.has_embed and not a.has_head and b.has_head and not b.has_embed
    for k in ("router", "experts_gate_up", "experts_down", "qkv", "q_norm"):
        assert torch.equal(getattr(whole.layers[0], k), getattr(a.layers[0], k))
        assert torch.equal(getattr(whole.layers[1], k), getattr(b.layers[0], k))
    eng = LLMEngine(EngineConfig(model="qwen3-moe-tiny", device="cpu", num_blocks=32, max_num_seqs=2,
                                 max_model_len=256, max_num_batched_tokens=64, use_graphs=False,
                                 enable_prefix_caching=False), model_cfg=c, model=whole)
    a.kv_cache = torch.zeros_like(whole.kv_cache[0:1])
    b.kv_cache = torch.zeros_like(whole.kv_cache[1:2])
    steps = []
    fwd = whole.forward

    def both(meta, input_ids=None, hidden=None):
        ref = fwd(meta, input_ids=input_ids, hidden=hidden)
        split = b.forward(meta, hidden=a.forward(meta, input_ids=input_ids))
        steps.append((input_ids.numel(), torch.equal(ref, split)))
        return ref
    whole.forward = both
    eng.generate([[1] + list(range(7, 40)), [1, 2, 3]], SamplingParams(max_tokens=3, temperature=0.0, ignore_eos=True))
    assert len(steps) >= 3 and max(n for n, _ in steps) >= 30 and min(n for n, _ in steps) <= 2
    assert all(ok for _, ok in steps), steps


def test_route_hook_records_and_forces():
    from dgi.engine import EngineConfig, LLMEngine
    from dgi.sched.request import SamplingParams
    c = get_config("qwen3-moe-tiny")
    m = LlamaModel(c, "cpu", torch.float32, seed=2)
    eng = LLMEngine(EngineConfig(model="qwen3-moe-tiny", device="cpu", dtype=torch.float32, num_blocks=32,
                                 max_num_seqs=2, max_model_len=256, max_num_batched_tokens=64, use_graphs=False,
                                 enable_prefix_caching=False), model_cfg=c, model=m)
    prompt = [1, 9, 8, 7, 6, 5]
    sp = SamplingParams(max_tokens=3, temperature=0.0, ignore_eos=True)
    base = eng.generate([prompt], sp)[0].output
    seen = {}

    def record(layer, positions, ids, weights):
        assert ids.shape == weights.shape == (positions.numel(), K)
        for r, p in enumerate(positions.tolist()):
            seen[(layer, p)] = ids[r].tolist()
        return None
    m.route_hook = record
    assert eng.generate([prompt], sp)[0].output == base
    assert {l for l, _ in seen} == {0, 1} and {p for _, p in seen} >= set(range(len(prompt) + 2))

    def force(layer, positions, ids, weights):
        return torch.tensor([seen[(layer, p)][::-1] for p in positions.tolist()], dtype=torch.int32)
    m.route_hook = force          # the same experts in the other order: the same function
    assert eng.generate([prompt], sp)[0].output == base
    calls = []

    def wrong(layer, positions, ids, weights):
        calls.append(layer)
        return (ids + 3) % E
    m.route_hook = wrong
    eng.generate([prompt], sp)
    assert calls


def test_prefix_caching_capture_taps_and_layer_hook_carry_over():
    """What the MLP block does not touch keeps working on a MoE model: a prompt served from the prefix
    cache gives the tokens it gave cold, EAGLE feature taps hold the residual stream of their layers,
    and the layer hook (the P/D layer-streamed migration) fires once per layer and step."""
    from dgi.engine import EngineConfig, LLMEngine
    from dgi.sched.request import SamplingParams
    c = get_config("qwen3-moe-tiny")
    m = LlamaModel(c, "cpu", torch.float32, seed=6)
    eng = LLMEngine(EngineConfig(model="qwen3-moe-tiny", device="cpu", dtype=torch.float32, num_blocks=64,
                                 max_num_seqs=2, max_model_len=256, max_num_batched_tokens=128, use_graphs=False,
                                 enable_prefix_caching=True), model_cfg=c, model=m)
    prompt = [1] + list(range(20, 90))
    sp = SamplingParams(max_tokens=4, temperature=0.0, ignore_eos=True)
    cold = eng.generate([prompt], sp)[0].output
    rows = []
    orig = ops.moe_mlp

    def counted(x, *a, **k):
        rows.append(x.shape[0])
        return orig(x, *a, **k)
    ops.moe_mlp = counted
    hooked = []
    m.layer_hook = hooked.append
    m.capture_layers = (0, 1)
    try:
        warm = eng.generate([prompt], sp)[0].output
    finally:
        ops.moe_mlp = orig
        m.layer_hook = None
        m.capture_layers = ()
    assert warm == cold
    assert max(rows) < len(prompt)                      # the cached prefix was not recomputed
    assert hooked[:2] == [0, 1] and len(hooked) == 2 * 4
    assert set(m.captured) == {0, 1} and m.captured[1].shape[-1] == c.hidden_size


def test_refusals():
    from dgi.engine import EngineConfig, LLMEngine
    from dgi.parallel.tensor import tp_local_config
    c = get_config("qwen3-moe-tiny")
    m = LlamaModel(c, "cpu", seed=0)
    for mode in ("fp8", "mxfp4"):
        with pytest.raises(ValueError, match="MoE"):
            m.quantize_weights(mode)
    with pytest.raises(ValueError, match="MoE"):
        LLMEngine(EngineConfig(model="qwen3-moe-tiny", device="cpu", num_blocks=16, max_num_seqs=2, max_model_len=64,
                               max_num_batched_tokens=64, use_graphs=False, weight_quant="fp8"))
    with pytest.raises(ValueError, match="MoE"):
        tp_local_config(c, 2)
    assert all(k in PRESETS for k in ("qwen3-30b-a3b", "qwen3-moe-tiny"))
