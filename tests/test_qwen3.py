"""Qwen3 on the CPU reference path: config translation and name resolution, the q/k-norm + RoPE
writer's definition against hand-written math, fp32 parity with Hugging Face ``Qwen3ForCausalLM``,
and the bookkeeping every per-layer tensor walk owes the two new gains.  (The HIP kernel and the
GPU engine: tests/test_qwen3_gpu.py.)"""
import hashlib
import math
import multiprocessing as mp
import os
import socket
import traceback

import pytest
import torch

from dgi import ops
from dgi.models.config import ModelConfig, get_config
from dgi.models.llama import QUANT_SLOTS, LlamaModel

# ---------------------------------------------------------------------------- configs and names

H, I, L, NH, NKV, HD, V = 256, 512, 2, 8, 2, 64, 512          # q_size = 512 != hidden


def _hf_config(**kw):
    transformers = pytest.importorskip("transformers")
    common = dict(vocab_size=V, hidden_size=H, intermediate_size=I, num_hidden_layers=L, num_attention_heads=NH,
                  num_key_value_heads=NKV, head_dim=HD, max_position_embeddings=512, rms_norm_eps=1e-6,
                  bos_token_id=1, eos_token_id=2, tie_word_embeddings=False, rope_theta=1000000.0)
    common.update(kw)
    return transformers.Qwen3Config(**common)


def test_config_translation():
    mc = ModelConfig.from_hf_dict(_hf_config().to_dict())
    assert mc.arch == "qwen3" and mc.qk_norm and not mc.qkv_bias
    assert (mc.hidden_size, mc.num_heads, mc.num_kv_heads, mc.head_dim) == (H, NH, NKV, HD)
    assert mc.q_size == 512 and mc.q_size != mc.hidden_size
    assert mc.rope_theta == 1e6            # transformers >= 5 nests theta under rope_parameters
    assert (mc.rope_dim, mc.rope_interleaved) == (HD, False)
    assert ModelConfig.from_hf_dict(_hf_config(attention_bias=True).to_dict()).qkv_bias
    # the other families keep the flag off
    assert not ModelConfig.from_hf_dict({"model_type": "qwen2", "hidden_size": 64, "num_attention_heads": 2,
                                         "vocab_size": 8, "intermediate_size": 8, "num_hidden_layers": 1}).qk_norm


def test_name_resolution():
    c = get_config("Qwen/Qwen3-8B")
    assert c.intermediate_size == 12288 and c.arch == "qwen3" and c.qk_norm and not c.qkv_bias
    assert (c.hidden_size, c.num_layers, c.num_heads, c.num_kv_heads, c.head_dim) == (4096, 36, 32, 8, 128)
    c = get_config("Qwen/Qwen3-32B")
    assert (c.hidden_size, c.intermediate_size, c.num_layers, c.num_heads, c.q_size) == (5120, 25600, 64, 64, 8192)
    c = get_config("Qwen/Qwen3-0.6B")
    assert (c.hidden_size, c.num_layers, c.num_heads, c.q_size, c.tie_embeddings) == (1024, 28, 16, 2048, True)
    # sizes are read from the name, qwen3 before qwen
    assert get_config("Qwen/Qwen3-8B-Base").num_layers == 36
    assert get_config("some/qwen3-0.6b-chat").hidden_size == 1024
    t = get_config("qwen3-tiny")
    assert t.q_size == 2 * t.hidden_size and t.qk_norm and t.tie_embeddings and t.vocab_size == 1024
    for c in (get_config(n) for n in ("qwen3-8b", "qwen3-32b", "qwen3-0.6b")):
        assert (c.vocab_size, c.rope_theta, c.rms_eps, c.max_position) == (151936, 1e6, 1e-6, 40960)
        assert (c.bos_token_id, c.eos_token_id) == (151643, 151645)


def test_qwen25_name_resolves_as_before():
    c = get_config("Qwen/Qwen2.5-7B-Instruct")
    assert (c.arch, c.intermediate_size, c.qkv_bias, c.qk_norm) == ("qwen2", 18944, True, False)
    assert get_config("Qwen/Qwen2.5-72B-something").intermediate_size == 18944      # the old family guess
    assert get_config("Qwen/Qwen2.5-0.5B").hidden_size == 896


@pytest.mark.parametrize("name", ["Qwen/Qwen3-30B-A3B", "Qwen/Qwen3-235B-A22B", "Qwen/Qwen3-14B", "Qwen/Qwen3-1.7B"])
def test_unknown_qwen3_size_raises(name):
    with pytest.raises(KeyError):
        get_config(name)


def test_sliding_window_config_raises():
    d = _hf_config().to_dict()
    ModelConfig.from_hf_dict(d)
    with pytest.raises(ValueError):
        ModelConfig.from_hf_dict({**d, "use_sliding_window": True})
    with pytest.raises(ValueError):
        ModelConfig.from_hf_dict({**d, "layer_types": ["full_attention", "sliding_attention"]})


def test_param_count_counts_the_gains():
    c = get_config("qwen3-tiny")
    m = LlamaModel(c, "cpu", seed=1)
    assert sum(t.numel() for _, t in m.tensors()) == c.param_count()
    plain = ModelConfig(**{**c.to_dict(), "qk_norm": False})
    assert c.param_count() - plain.param_count() == c.num_layers * 2 * c.head_dim


# ---------------------------------------------------------------------------- the definition

def test_reference_matches_hand_written_math():
    """One token, fp32.  Every head has its own input scale, one q head and the k head are scaled by
    2^-10 so that eps decides their result (mean square ~ 1e-6 = eps): a norm taken over the wrong
    span (all heads, or a neighbouring head) and a missing eps both land far outside the bound."""
    nh, nkv, hd, eps, theta, pos, bs = 3, 2, 16, 1e-6, 10000.0, 37, 4
    g = torch.Generator().manual_seed(4)
    x = torch.randn(nh + 2 * nkv, hd, generator=g, dtype=torch.float64)
    scales = torch.tensor([4.0, 2.0 ** -10, 0.5, 2.0 ** -10, 8.0, 1.0, 3.0], dtype=torch.float64)
    x = x * scales[:, None]
    qg = 0.25 + 3.75 * torch.rand(hd, generator=g, dtype=torch.float64)
    kg = 0.25 + 3.75 * torch.rand(hd, generator=g, dtype=torch.float64)
    want = []
    for h in range(nh + nkv):
        gain = qg if h < nh else kg
        ms = sum(float(x[h, d]) ** 2 for d in range(hd)) / hd
        n = [float(x[h, d]) / math.sqrt(ms + eps) * float(gain[d]) for d in range(hd)]
        o = [0.0] * hd
        for i in range(hd // 2):
            a = pos * theta ** (-2.0 * i / hd)
            o[i] = n[i] * math.cos(a) - n[i + hd // 2] * math.sin(a)
            o[i + hd // 2] = n[i + hd // 2] * math.cos(a) + n[i] * math.sin(a)
        want.append(o)
    want = torch.tensor(want, dtype=torch.float64)
    # the two tiny heads: eps halves (roughly) what a norm without eps would give
    assert 0.3 < float(want[1].abs().max() / (x[1] / x[1].pow(2).mean().sqrt() * qg).abs().max()) < 0.9

    qkv = x.reshape(1, -1).float()
    kc = torch.full((3, nkv, bs, hd), 7.0)
    vc = torch.full((3, nkv, bs, hd), 7.0)
    cs = ops.rope_cos_sin(hd, 64, theta)
    ops.qknorm_rope_cache(qkv, torch.tensor([pos], dtype=torch.int32), cs, qg.float(), kg.float(), eps, nh, nkv, hd,
                          torch.tensor([9], dtype=torch.int32), kc, vc)
    torch.testing.assert_close(qkv[0, : nh * hd].double().view(nh, hd), want[:nh], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(kc[2, :, 1].double(), want[nh:], rtol=1e-5, atol=1e-6)
    assert torch.equal(vc[2, :, 1], x[nh + nkv:].float())                     # v untouched
    kc[2, :, 1] = 7.0
    vc[2, :, 1] = 7.0
    assert bool((kc == 7.0).all()) and bool((vc == 7.0).all())                # nothing else written


def test_reference_skips_negative_slots_and_takes_any_geometry():
    """The reference is a composition: partial interleaved rotary over 96-dim heads works, and a
    slot < 0 writes no page while q is still normalised and rotated."""
    nh, nkv, hd, rd = 2, 1, 96, 32
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(2, (nh + 2 * nkv) * hd, generator=g)
    q0 = qkv.clone()
    kc, vc = torch.zeros(2, nkv, 4, hd), torch.zeros(2, nkv, 4, hd)
    ops.qknorm_rope_cache_ref(qkv, torch.tensor([3, 5]), ops.rope_cos_sin(rd, 16, 1e4), torch.ones(hd), torch.ones(hd),
                              1e-6, nh, nkv, hd, torch.tensor([-1, 6]), kc, vc, mode=1)
    assert int((kc != 0).any(-1).sum()) == 1 and bool((kc[1, 0, 2] != 0).all())
    assert not torch.equal(qkv[0, : nh * hd], q0[0, : nh * hd])
    # the pass-through dims are the normalised input
    torch.testing.assert_close(qkv[1, rd:hd], ops.rmsnorm_ref(q0[1, :hd], torch.ones(hd), 1e-6)[rd:])


# ---------------------------------------------------------------------------- HF parity (fp32)

def _hf_model():
    transformers = pytest.importorskip("transformers")
    cfg = _hf_config()
    model = transformers.Qwen3ForCausalLM(cfg)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "q_norm" in n or "k_norm" in n:
                # far from one: a dropped or swapped gain moves the logits by their own size
                p.copy_(0.25 + 3.75 * torch.rand(p.shape, generator=g))
            elif "norm" in n:
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
    return model.eval(), cfg


def _native_engine(cfg, model):
    from dgi.engine import EngineConfig, LLMEngine
    mc = ModelConfig.from_hf_dict(cfg.to_dict(), name="hf-tiny")
    nm = LlamaModel(mc, "cpu", torch.float32, init="empty")
    nm.load_state_dict_hf(model.state_dict())
    eng = LLMEngine(EngineConfig(model="hf-tiny", device="cpu", dtype=torch.float32, num_blocks=64, max_num_seqs=4,
                                 max_model_len=256, max_num_batched_tokens=64, use_graphs=False,
                                 enable_prefix_caching=False), model_cfg=mc, model=nm)
    return mc, eng


def test_greedy_continuation_matches_hf():
    from dgi.sched.request import SamplingParams
    model, cfg = _hf_model()
    _, eng = _native_engine(cfg, model)
    prompts = [[1, 17, 99, 250, 3, 77, 401, 12, 8, 300, 45], [1, 5, 6]]
    n_new = 8
    reqs = eng.generate(prompts, SamplingParams(max_tokens=n_new, temperature=0.0, ignore_eos=True))
    for p, r in zip(prompts, reqs):
        with torch.no_grad():
            ref = model.generate(torch.tensor([p]), max_new_tokens=n_new, do_sample=False, min_new_tokens=n_new,
                                 pad_token_id=0)[0, len(p):].tolist()
        assert r.output == ref, (r.output, ref)


def test_prefill_logits_match_hf():
    from dgi.sched.request import SamplingParams
    model, cfg = _hf_model()
    mc, eng = _native_engine(cfg, model)
    assert mc.qk_norm and mc.q_size != mc.hidden_size
    prompt = [1, 33, 44, 55, 66, 77, 88, 99, 111, 222]
    with torch.no_grad():
        ref = model(torch.tensor([prompt])).logits[0, -1]
    captured = {}
    orig = eng.model.compute_logits

    def spy(h, residual, idx):
        out = orig(h, residual, idx)
        captured["logits"] = out.detach().clone()
        return out

    eng.model.compute_logits = spy
    eng.generate([prompt], SamplingParams(max_tokens=1, temperature=0.0, ignore_eos=True))
    got = captured["logits"][-1]
    print("max |native - hf| logit:", float((got - ref).abs().max()), "max |hf|:", float(ref.abs().max()))
    torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-4)


def test_state_dict_without_the_gains_is_an_error():
    model, cfg = _hf_model()
    sd = {k: v for k, v in model.state_dict().items() if "q_norm" not in k}
    nm = LlamaModel(ModelConfig.from_hf_dict(cfg.to_dict()), "cpu", torch.float32, init="empty")
    with pytest.raises(KeyError):
        nm.load_state_dict_hf(sd)


def test_safetensors_checkpoint_loads_the_gains_and_refuses_one_without(tmp_path):
    pytest.importorskip("safetensors")
    from safetensors.torch import save_file
    model, cfg = _hf_model()
    model.save_pretrained(str(tmp_path / "ok"), safe_serialization=True)
    mc = ModelConfig.from_file(str(tmp_path / "ok"))
    assert mc.qk_norm
    nm = LlamaModel(mc, "cpu", torch.float32, checkpoint=str(tmp_path / "ok"))
    sd = model.state_dict()
    for i, Lw in enumerate(nm.layers):
        assert torch.equal(Lw.q_norm, sd[f"model.layers.{i}.self_attn.q_norm.weight"])
        assert torch.equal(Lw.k_norm, sd[f"model.layers.{i}.self_attn.k_norm.weight"])
    assert nm.load_info["tensors"] == L * 11 + 3
    os.makedirs(tmp_path / "bad")
    save_file({k: v.contiguous() for k, v in sd.items() if "k_norm" not in k}, str(tmp_path / "bad" / "model.safetensors"))
    with pytest.raises(KeyError):
        LlamaModel(mc, "cpu", torch.float32, checkpoint=str(tmp_path / "bad"))


# ---------------------------------------------------------------------------- composition and bookkeeping

PROMPTS = [[1] + list(range(7, 7 + n)) for n in (3, 40)]


def _tiny_tokens(model, **kw):
    from dgi.engine import EngineConfig, LLMEngine
    from dgi.sched.request import SamplingParams
    eng = LLMEngine(EngineConfig(model="qwen3-tiny", device="cpu", dtype=model.dtype, num_blocks=64, max_num_seqs=4,
                                 max_model_len=256, max_num_batched_tokens=64, use_graphs=False,
                                 enable_prefix_caching=False, **kw), model_cfg=model.cfg, model=model)
    return [r.output for r in eng.generate(PROMPTS, SamplingParams(max_tokens=6, temperature=0.0, ignore_eos=True))]


def _spy_method(obj, name):
    calls = []
    orig = getattr(obj, name)

    def wrapped(*a, **k):
        calls.append(1)
        return orig(*a, **k)
    setattr(obj, name, wrapped)
    return calls


def test_fused_and_folded_layer_loops_produce_the_unfused_tokens(monkeypatch):
    from dgi.models import llama
    mc = get_config("qwen3-tiny")
    src = LlamaModel(mc, "cpu", torch.float32, seed=11)
    want = _tiny_tokens(src)
    fused = LlamaModel(mc, "cpu", torch.float32, init="empty").copy_from(src)
    fused.force_fused = True
    ran = _spy_method(fused, "_forward_layers_fused")
    assert _tiny_tokens(fused) == want and ran
    fold = LlamaModel(mc, "cpu", torch.float32, init="empty").copy_from(src)
    monkeypatch.setattr(llama, "NORM_FOLD", "force-cpu")
    monkeypatch.setattr(llama, "NORM_FOLD_MIN_ROWS", 1)
    ran = _spy_method(fold, "_forward_layers_folded")
    assert _tiny_tokens(fold) == want and ran
    assert fold.norms_folded
    for Lw, Ls in zip(fold.layers, src.layers):      # fold_norms leaves the per-head gains alone
        assert torch.equal(Lw.q_norm, Ls.q_norm) and torch.equal(Lw.k_norm, Ls.k_norm)


def test_attention_refuses_a_rope_epilogue_before_the_norm():
    m = LlamaModel(get_config("qwen3-tiny"), "cpu", torch.float32, seed=1)
    m.kv_cache = torch.zeros(2, 2, 2, 2, 16, 128)
    with pytest.raises(RuntimeError):
        m.attention(0, torch.zeros(1, m.cfg.qkv_size), None, rope=False)


@pytest.mark.parametrize("mode", ["fp8", "mxfp4"])
def test_quantize_weights_leaves_the_gains(mode):
    mc = get_config("qwen3-tiny")
    src = LlamaModel(mc, "cpu", seed=2)
    m = LlamaModel(mc, "cpu", init="empty").copy_from(src)
    before = m.weight_bytes()
    m.quantize_weights(mode)
    kind = ops.Fp8Weight if mode == "fp8" else ops.Mxfp4Weight
    for Lw, Ls in zip(m.layers, src.layers):
        assert all(isinstance(getattr(Lw, k), kind) for k in QUANT_SLOTS)
        for k in ("q_norm", "k_norm"):
            t = getattr(Lw, k)
            assert t.dtype == torch.bfloat16 and tuple(t.shape) == (mc.head_dim,) and torch.equal(t, getattr(Ls, k))
    assert m.weight_bytes() < before
    assert len(_tiny_tokens(m)[0]) == 6       # the quantised loop runs with the norm


def test_copy_from_tensors_and_weight_bytes_carry_the_gains():
    mc = get_config("qwen3-tiny")
    src = LlamaModel(mc, "cpu", seed=3)
    names = dict(src.tensors())
    for i in range(mc.num_layers):
        assert tuple(names[f"layers.{i}.q_norm"].shape) == (mc.head_dim,)
        assert tuple(names[f"layers.{i}.k_norm"].shape) == (mc.head_dim,)
    assert not torch.equal(src.layers[0].q_norm, src.layers[0].k_norm)
    assert not torch.equal(src.layers[0].q_norm, torch.ones(mc.head_dim, dtype=torch.bfloat16))
    dst = LlamaModel(mc, "cpu", init="empty")
    assert torch.equal(dst.layers[0].q_norm, torch.ones(mc.head_dim, dtype=torch.bfloat16))
    dst.copy_from(src)
    for a, b in zip(dst.layers, src.layers):
        assert torch.equal(a.q_norm, b.q_norm) and torch.equal(a.k_norm, b.k_norm)
    assert src.weight_bytes() == 2 * mc.param_count()
    assert all(Lw.q_norm is None and Lw.k_norm is None for Lw in LlamaModel(get_config("qwen-tiny"), "cpu").layers)


def _weights_sha256(name, seed):
    m = LlamaModel(get_config(name), "cpu", seed=seed)
    h = hashlib.sha256()
    for n, t in m.tensors():
        h.update(n.encode())
        h.update(t.contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


# recorded with this function on the commit before the q/k gains were added (seed 3, CPU, bf16)
PARENT_SHA256 = {"llama-tiny": "4c7476967b7f3b89de28f6e7c0bdae8d62cd178ab740264c866933539488b6d1",
                 "qwen-tiny": "cf62bca51a1579512d7be42770fcd4f7f896ed9feca6b2f5704823bf29844d9c"}


@pytest.mark.parametrize("name", sorted(PARENT_SHA256))
def test_existing_models_keep_their_random_weights(name):
    assert _weights_sha256(name, 3) == PARENT_SHA256[name]


# ---------------------------------------------------------------------------- tensor parallel

def _tp_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    try:
        import torch.distributed as dist
        from dgi.engine import EngineConfig, LLMEngine
        from dgi.parallel.fabric import init_distributed
        from dgi.parallel.tensor import TPEngine
        from dgi.sched.request import SamplingParams
        init_distributed("gloo")
        cfg = EngineConfig(model="qwen3-tiny", device="cpu", num_blocks=None, max_num_seqs=4, max_model_len=256,
                           max_num_batched_tokens=128, use_graphs=False, enable_prefix_caching=True)
        g = torch.Generator().manual_seed(0)
        prompts = [torch.randint(5, 500, (n,), generator=g).tolist() for n in (9, 17, 30)]
        sp = SamplingParams(max_tokens=8, temperature=0.0, ignore_eos=True)
        eng = TPEngine(cfg, rank, world)
        assert eng.model.cfg.num_kv_heads == 1 and eng.model.layers[0].q_norm.shape[0] == 128
        out = [r.output for r in eng.generate(prompts, sp)]
        if rank == 0:
            ref_eng = LLMEngine(cfg)
            assert torch.equal(ref_eng.model.layers[1].k_norm, eng.model.layers[1].k_norm)
            ref = [r.output for r in ref_eng.generate(prompts, sp)]
            assert out == ref, (out, ref)
        q.put((rank, "ok", out))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        q.put((rank, "err", traceback.format_exc()))


def test_tensor_parallel_matches_single_process():
    """TP=2 over qwen3-tiny's 2 KV heads equals TP=1 (as test_parallel_cpu does for llama-tiny-tp):
    every rank holds the per-head gains whole."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_tp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        for _ in range(2):
            rank, status, res = q.get(timeout=240)
            assert status == "ok", f"rank {rank} failed:\n{res}"
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
