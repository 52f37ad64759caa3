"""Sliding-window attention on the CPU: the references against a dense masked softmax in fp64,
config translation (Mistral, Qwen2), HF parity in fp32, checkpoints, layer ranges, the prefix
cache and the refusals.

The rule (HF ``masking_utils.sliding_window_overlay``): with a window W > 0 the query at absolute
position p sees key j iff j <= p and j > p - W — W keys, its own included; W = 0 is full attention.
"""
import dataclasses
import math

import pytest
import torch

from dgi import ops
from dgi.models.config import ModelConfig, get_config
from dgi.models.llama import LlamaModel

WINDOWS = [1, 16, 33, 40, 64]


# ---------------------------------------------------------------------------- references

def _pool(ctxs, nkv, hd, bs, gen):
    """A shuffled paged pool holding ctxs[b] random tokens per sequence."""
    need = [(c + bs - 1) // bs for c in ctxs]
    nblk = 1 + sum(need)
    ids = (torch.randperm(nblk - 1, generator=gen) + 1).tolist()
    kc = torch.randn(nblk, nkv, bs, hd, generator=gen)
    vc = torch.randn(nblk, nkv, bs, hd, generator=gen)
    bt = torch.zeros(len(ctxs), max(need) + 1, dtype=torch.int32)
    k0 = 0
    for b, n in enumerate(need):
        bt[b, :n] = torch.tensor(ids[k0:k0 + n], dtype=torch.int32)
        k0 += n
    return kc, vc, bt


def _dense(q, kc, vc, bt, qlens, ctxs, nh, nkv, scale, window):
    """fp64 softmax over the dense [qlen, ctx] mask j <= p and (W == 0 or j > p - W)."""
    hd, bs, G = kc.shape[-1], kc.shape[2], nh // nkv
    out = torch.zeros(sum(qlens), nh * hd, dtype=torch.float64)
    r0 = 0
    for b, (ql, ctx) in enumerate(zip(qlens, ctxs)):
        if ql == 0:
            continue
        t = torch.arange(ctx)
        blk = bt[b].long()[t // bs]
        k = kc[blk, :, t % bs].double()                      # [ctx, nkv, hd]
        v = vc[blk, :, t % bs].double()
        qb = q[r0:r0 + ql, : nh * hd].double().view(ql, nkv, G, hd)
        s = torch.einsum("qhgd,thd->hgqt", qb, k) * scale
        p = torch.arange(ctx - ql, ctx)[:, None]
        j = t[None, :]
        allow = j <= p
        if window > 0:
            allow = allow & (j > p - window)
        assert int(allow.sum(1).min()) == (min(window, ctx - ql + 1) if window else ctx - ql + 1)
        s = s.masked_fill(~allow[None, None], -math.inf)
        o = torch.einsum("hgqt,thd->qhgd", torch.softmax(s, -1), v)
        out[r0:r0 + ql] = o.reshape(ql, -1)
        r0 += ql
    return out


def _ctxs(W):
    return sorted({c for c in (1, W - 1, W, W + 1, 2 * W + 5) if c >= 1})


@pytest.mark.parametrize("W", WINDOWS)
def test_decode_ref_matches_dense_fp64(W):
    nh, nkv, hd, bs = 4, 2, 16, 8
    gen = torch.Generator().manual_seed(W)
    ctxs = _ctxs(W)
    kc, vc, bt = _pool(ctxs, nkv, hd, bs, gen)
    q = torch.randn(len(ctxs), nh * hd, generator=gen)
    ctx = torch.tensor(ctxs, dtype=torch.int32)
    got = ops.paged_decode_ref(q, kc, vc, bt, ctx, nh, nkv, 0.25, window=W)
    want = _dense(q, kc, vc, bt, [1] * len(ctxs), ctxs, nh, nkv, 0.25, W)
    torch.testing.assert_close(got.double(), want, rtol=1e-5, atol=1e-6)
    # the public op is the reference on the CPU
    assert torch.equal(ops.paged_decode(q, kc, vc, bt, ctx, nh, nkv, 0.25, window=W), got)
    if W > 1:      # the window is not a no-op on the longest context
        full = ops.paged_decode_ref(q, kc, vc, bt, ctx, nh, nkv, 0.25)
        assert not torch.allclose(got[-1], full[-1], atol=1e-3)


@pytest.mark.parametrize("W", WINDOWS)
def test_prefill_ref_matches_dense_fp64(W):
    nh, nkv, hd, bs = 4, 2, 16, 8
    gen = torch.Generator().manual_seed(100 + W)
    # (qlen, ctx): whole prompts, and chunks behind a cached prefix that straddles the window:
    # shorter than W, exactly W - 1 / W / W + 1, and far longer
    pairs = [(c, c) for c in _ctxs(W)]
    pairs += [(7, 7 + pre) for pre in sorted({max(W - 3, 0), max(W - 1, 0), W, W + 1, 2 * W + 5})]
    pairs += [(W + 9, 2 * W + 20), (0, 5)]
    qlens, ctxs = [p[0] for p in pairs], [p[1] for p in pairs]
    kc, vc, bt = _pool(ctxs, nkv, hd, bs, gen)
    q = torch.randn(sum(qlens), nh * hd, generator=gen)
    cu = torch.tensor([0] + list(torch.tensor(qlens).cumsum(0)), dtype=torch.int32)
    ctx = torch.tensor(ctxs, dtype=torch.int32)
    got = ops.paged_prefill_ref(q, kc, vc, bt, cu, ctx, nh, nkv, 0.25, window=W)
    want = _dense(q, kc, vc, bt, qlens, ctxs, nh, nkv, 0.25, W)
    torch.testing.assert_close(got.double(), want, rtol=1e-5, atol=1e-6)
    assert torch.equal(ops.paged_prefill(q, kc, vc, bt, cu, ctx, nh, nkv, 0.25, window=W), got)


def test_no_window_is_bit_equal_to_the_call_without_the_argument():
    nh, nkv, hd, bs = 4, 2, 16, 8
    gen = torch.Generator().manual_seed(7)
    ctxs = [1, 9, 40, 77]
    kc, vc, bt = _pool(ctxs, nkv, hd, bs, gen)
    ctx = torch.tensor(ctxs, dtype=torch.int32)
    q = torch.randn(len(ctxs), nh * hd, generator=gen)
    base = ops.paged_decode_ref(q, kc, vc, bt, ctx, nh, nkv, 0.25)
    for W in (0, 77, 78, 1 << 20):
        assert torch.equal(ops.paged_decode_ref(q, kc, vc, bt, ctx, nh, nkv, 0.25, window=W), base)
        assert torch.equal(ops.paged_decode(q, kc, vc, bt, ctx, nh, nkv, 0.25, window=W), base)
    qlens = [1, 4, 40, 30]
    qp = torch.randn(sum(qlens), nh * hd, generator=gen)
    cu = torch.tensor([0, 1, 5, 45, 75], dtype=torch.int32)
    base = ops.paged_prefill_ref(qp, kc, vc, bt, cu, ctx, nh, nkv, 0.25)
    for W in (0, 77, 78, 1 << 20):
        assert torch.equal(ops.paged_prefill_ref(qp, kc, vc, bt, cu, ctx, nh, nkv, 0.25, window=W), base)
        assert torch.equal(ops.paged_prefill(qp, kc, vc, bt, cu, ctx, nh, nkv, 0.25, window=W), base)


def test_negative_window_and_window_with_a_tree_are_refused():
    nh, nkv, hd, bs = 4, 2, 16, 8
    gen = torch.Generator().manual_seed(8)
    kc, vc, bt = _pool([12], nkv, hd, bs, gen)
    ctx = torch.tensor([12], dtype=torch.int32)
    q = torch.randn(1, nh * hd, generator=gen)
    qp = torch.randn(4, nh * hd, generator=gen)
    cu = torch.tensor([0, 4], dtype=torch.int32)
    for fn in (ops.paged_decode, ops.paged_decode_ref):
        with pytest.raises(ValueError, match="window"):
            fn(q, kc, vc, bt, ctx, nh, nkv, 0.25, window=-1)
    for fn in (ops.paged_prefill, ops.paged_prefill_ref):
        with pytest.raises(ValueError, match="window"):
            fn(qp, kc, vc, bt, cu, ctx, nh, nkv, 0.25, window=-4)
    tm = ops.tree_mask_ref(torch.tensor([[-1, 0, 0, 1]], dtype=torch.int32))[0]
    with pytest.raises(ValueError, match="tree"):
        ops.paged_prefill(qp, kc, vc, bt, cu, ctx, nh, nkv, 0.25, tree_mask=tm, tree_n=4, window=8)
    with pytest.raises(ValueError, match="tree"):
        ops.paged_prefill_ref(qp, kc, vc, bt, cu, ctx, nh, nkv, 0.25, tm, 4, window=8)


# ---------------------------------------------------------------------------- configuration

BASE = {"hidden_size": 64, "num_attention_heads": 4, "num_key_value_heads": 2, "vocab_size": 128,
        "intermediate_size": 96, "num_hidden_layers": 2}


def test_mistral_config_translation():
    mc = ModelConfig.from_hf_dict({**BASE, "model_type": "mistral", "sliding_window": 4096})
    assert (mc.arch, mc.sliding_window, mc.window_layers, mc.qkv_bias) == ("llama", 4096, None, False)
    assert [mc.window_of(i) for i in range(2)] == [4096, 4096] and mc.has_window
    mc = ModelConfig.from_hf_dict({**BASE, "model_type": "mistral", "sliding_window": None})
    assert (mc.arch, mc.sliding_window) == ("llama", 0) and not mc.has_window and mc.window_of(1) == 0
    # a Llama config never slides, whatever key it carries
    assert not ModelConfig.from_hf_dict({**BASE, "model_type": "llama", "sliding_window": 64}).has_window


def test_qwen2_config_translation():
    d = {**BASE, "model_type": "qwen2", "sliding_window": 40, "max_window_layers": 1}
    off = ModelConfig.from_hf_dict({**d, "use_sliding_window": False})
    assert off.arch == "qwen2" and off.sliding_window == 0 and not off.has_window
    on = ModelConfig.from_hf_dict({**d, "use_sliding_window": True})
    assert (on.sliding_window, on.window_layers) == (40, (1,))
    assert [on.window_of(i) for i in range(2)] == [0, 40]
    # max_window_layers at the layer count: no layer slides
    assert not ModelConfig.from_hf_dict({**d, "use_sliding_window": True, "max_window_layers": 2}).has_window


def test_layer_types_take_precedence():
    d = {**BASE, "model_type": "qwen2", "sliding_window": 40, "max_window_layers": 1, "use_sliding_window": True}
    mc = ModelConfig.from_hf_dict({**d, "layer_types": ["sliding_attention", "full_attention"]})
    assert [mc.window_of(i) for i in range(2)] == [40, 0]
    mc = ModelConfig.from_hf_dict({**d, "layer_types": ["full_attention", "full_attention"]})
    assert not mc.has_window
    m = {**BASE, "model_type": "mistral", "sliding_window": 16}
    mc = ModelConfig.from_hf_dict({**m, "layer_types": ["full_attention", "sliding_attention"]})
    assert [mc.window_of(i) for i in range(2)] == [0, 16]
    assert ModelConfig.from_hf_dict({**m, "layer_types": ["sliding_attention"] * 2}).window_layers is None
    with pytest.raises(ValueError):
        ModelConfig.from_hf_dict({**m, "layer_types": ["sliding_attention", "chunked_attention"]})
    with pytest.raises(ValueError):
        ModelConfig.from_hf_dict({**m, "sliding_window": None, "layer_types": ["sliding_attention"] * 2})


def test_presets_and_truncation():
    c = get_config("mistralai/Mistral-7B-v0.1")
    assert c.name == "mistral-7b" and c.arch == "llama" and c.sliding_window == 4096 and c.window_layers is None
    assert (c.num_layers, c.hidden_size, c.intermediate_size, c.num_heads, c.num_kv_heads, c.head_dim) == \
        (32, 4096, 14336, 32, 8, 128)
    assert (c.vocab_size, c.rope_theta, c.rms_eps, c.bos_token_id, c.eos_token_id) == (32000, 1e4, 1e-5, 1, 2)
    assert all(c.window_of(i) == 4096 for i in range(32))
    t = get_config("mistral-tiny")
    assert t.num_layers == 2 and [t.window_of(i) for i in range(2)] == [40, 40]
    s = get_config("qwen-tiny-swa")
    q = get_config("qwen-tiny")
    assert [s.window_of(i) for i in range(2)] == [0, 40]
    assert dataclasses.replace(s, name=q.name, sliding_window=0, window_layers=None) == q
    # <model>@L<n> keeps windows by global index
    assert [get_config("qwen-tiny-swa@L1").window_of(i) for i in range(2)] == [0, 40]
    assert not get_config("qwen-tiny-swa@L1").has_window
    m4 = get_config("mistral-7b@L4")
    assert m4.num_layers == 4 and all(m4.window_of(i) == 4096 for i in range(4))
    # no other preset slides
    from dgi.models.config import PRESETS
    assert sorted(k for k, v in PRESETS.items() if v.has_window) == ["mistral-7b", "mistral-tiny", "qwen-tiny-swa"]


# ---------------------------------------------------------------------------- HF parity (fp32)

W_HF = 40
HF_COMMON = dict(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=8,
                 num_key_value_heads=2, max_position_embeddings=512, rms_norm_eps=1e-6, bos_token_id=1,
                 eos_token_id=2, tie_word_embeddings=False)


def _hf_model(kind):
    transformers = pytest.importorskip("transformers")
    if kind == "mistral":
        cfg = transformers.MistralConfig(**HF_COMMON, head_dim=32, sliding_window=W_HF, rope_theta=10000.0)
        model = transformers.MistralForCausalLM(cfg)
    else:
        cfg = transformers.Qwen2Config(**HF_COMMON, use_sliding_window=True, sliding_window=W_HF,
                                       max_window_layers=1, rope_theta=1000000.0)
        model = transformers.Qwen2ForCausalLM(cfg)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "norm" in n:
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
    return model.eval(), cfg


def _native_engine(mc, state_dict, prefix_caching=False):
    from dgi.engine import EngineConfig, LLMEngine
    nm = LlamaModel(mc, "cpu", torch.float32, init="empty")
    nm.load_state_dict_hf(state_dict)
    return LLMEngine(EngineConfig(model=mc.name, device="cpu", dtype=torch.float32, num_blocks=64, max_num_seqs=4,
                                  max_model_len=256, max_num_batched_tokens=32, use_graphs=False,
                                  enable_prefix_caching=prefix_caching), model_cfg=mc, model=nm)


def _run(eng, prompt, n_new):
    """(logits of the last prompt position, greedy tokens) of a prompt prefilled in 32-token chunks."""
    from dgi.sched.request import SamplingParams
    seen = []
    orig = eng.model.compute_logits

    def spy(h, residual, idx):
        out = orig(h, residual, idx)
        seen.append(out.detach().clone())
        return out

    eng.model.compute_logits = spy
    try:
        req = eng.generate([prompt], SamplingParams(max_tokens=n_new, temperature=0.0, ignore_eos=True))[0]
    finally:
        eng.model.compute_logits = orig
    chunks = (len(prompt) + 31) // 32       # only the chunk that ends the prompt produces a logits row
    assert len(seen) == chunks + n_new - 1 and [l.shape[0] for l in seen] == [0] * (chunks - 1) + [1] * n_new
    return seen[chunks - 1][0], req.output


def _prompt(n=100):
    g = torch.Generator().manual_seed(3)
    return [1] + torch.randint(3, 500, (n - 1,), generator=g).tolist()


@pytest.mark.parametrize("kind", ["mistral", "qwen2"])
def test_hf_parity_and_the_unwindowed_control(kind):
    model, cfg = _hf_model(kind)
    mc = ModelConfig.from_hf_dict(cfg.to_dict(), name="hf-tiny-" + kind)
    assert [mc.window_of(i) for i in range(2)] == ([W_HF, W_HF] if kind == "mistral" else [0, W_HF])
    prompt, n_new = _prompt(100), 24
    with torch.no_grad():
        ref_all = model(torch.tensor([prompt])).logits[0]
        ids, ref_tokens = list(prompt), []
        for _ in range(n_new):          # full forward per token: no HF cache in the reference
            ref_tokens.append(int(model(torch.tensor([ids])).logits[0, -1].argmax()))
            ids.append(ref_tokens[-1])
    ref = ref_all[-1]
    got, tokens = _run(_native_engine(mc, model.state_dict()), prompt, n_new)
    print("max |native - hf| logit:", float((got - ref).abs().max()), "max |hf|:", float(ref.abs().max()))
    torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-4)
    assert tokens == ref_tokens, (tokens, ref_tokens)
    # short prompts inside the window: same bounds (the window must not bite early)
    short = prompt[:W_HF]
    with torch.no_grad():
        ref_s = model(torch.tensor([short])).logits[0, -1]
    got_s, _ = _run(_native_engine(mc, model.state_dict()), short, 1)
    torch.testing.assert_close(got_s, ref_s, rtol=1e-4, atol=1e-4)
    # control: the same weights served with full attention differ from HF past position 40, by far
    # more than the bound above (this is what a dropped window looks like)
    full = dataclasses.replace(mc, sliding_window=0, window_layers=None)
    got_f, _ = _run(_native_engine(full, model.state_dict()), prompt, 1)
    diff = float((got_f - ref).abs().max())
    print("max |unwindowed native - hf| logit:", diff)
    assert diff > 1e-2
    got_fs, _ = _run(_native_engine(full, model.state_dict()), short, 1)
    torch.testing.assert_close(got_fs, ref_s, rtol=1e-4, atol=1e-4)


def test_safetensors_mistral_checkpoint_loads(tmp_path):
    pytest.importorskip("safetensors")
    model, cfg = _hf_model("mistral")
    model.save_pretrained(str(tmp_path / "m"), safe_serialization=True)
    mc = ModelConfig.from_file(str(tmp_path / "m"))
    assert mc.arch == "llama" and mc.sliding_window == W_HF and mc.window_layers is None and mc.head_dim == 32
    nm = LlamaModel(mc, "cpu", torch.float32, checkpoint=str(tmp_path / "m"))
    ref = LlamaModel(mc, "cpu", torch.float32, init="empty")
    ref.load_state_dict_hf(model.state_dict())
    for a, b in zip(nm.layers, ref.layers):
        assert torch.equal(a.qkv, b.qkv) and torch.equal(a.o, b.o)


# ---------------------------------------------------------------------------- model and engine

def _windows_seen(monkeypatch):
    seen = []
    for name in ("paged_decode", "paged_prefill"):
        orig = getattr(ops, name)

        def spy(*a, _orig=orig, _name=name, **k):
            seen.append((_name, k.get("window", 0)))
            return _orig(*a, **k)
        monkeypatch.setattr(ops, name, spy)
    return seen


def test_layer_range_windows_by_global_index(monkeypatch):
    from dgi.engine import EngineConfig, LLMEngine
    from dgi.sched.request import SamplingParams
    mc = get_config("qwen-tiny-swa")
    mc = dataclasses.replace(mc, hidden_size=128, intermediate_size=128, num_heads=2, num_kv_heads=1, head_dim=64,
                             vocab_size=64)
    seen = _windows_seen(monkeypatch)
    for (a, b), want in (((1, 2), {40}), ((0, 1), {0}), ((0, 2), {0, 40})):
        del seen[:]
        m = LlamaModel(mc, "cpu", torch.float32, a, b, has_embed=True, has_head=True)
        assert m.num_local_layers == b - a
        eng = LLMEngine(EngineConfig(model=mc.name, device="cpu", dtype=torch.float32, num_blocks=16, max_num_seqs=2,
                                     max_model_len=64, max_num_batched_tokens=32, use_graphs=False, layer_start=a,
                                     layer_end=b), model_cfg=mc, model=m)
        eng.generate([[1, 5, 6, 7]], SamplingParams(max_tokens=2, temperature=0.0, ignore_eos=True))
        assert {w for _, w in seen} == want and {n for n, _ in seen} == {"paged_decode", "paged_prefill"}


def test_prefix_cache_on_and_off_give_the_same_tokens(monkeypatch):
    from dgi.engine import EngineConfig, LLMEngine
    from dgi.sched.request import SamplingParams
    mc = dataclasses.replace(get_config("mistral-tiny"), hidden_size=128, intermediate_size=128, num_heads=4,
                             num_kv_heads=2, head_dim=32, vocab_size=512)
    src = LlamaModel(mc, "cpu", torch.float32, seed=3)
    shared = _prompt(70)                       # a prefix longer than the 40-token window
    prompts = [shared + [7, 8, 9], shared + [11, 12], shared[:48] + [5]]
    sp = SamplingParams(max_tokens=12, temperature=0.0, ignore_eos=True)
    calls = []                                 # (window, cached prefix of the chunk) of every prefill launch
    orig = ops.paged_prefill

    def spy(q, kc, vc, bt, cu, ctx, *a, **k):
        calls.append((k.get("window", 0), int(ctx[0]) - int(cu[1] - cu[0])))
        return orig(q, kc, vc, bt, cu, ctx, *a, **k)
    monkeypatch.setattr(ops, "paged_prefill", spy)
    outs, first_prefix = [], []
    for caching in (False, True):
        m = LlamaModel(mc, "cpu", torch.float32, init="empty").copy_from(src)
        eng = LLMEngine(EngineConfig(model=mc.name, device="cpu", dtype=torch.float32, num_blocks=64, max_num_seqs=4,
                                     max_model_len=256, max_num_batched_tokens=32, use_graphs=False,
                                     enable_prefix_caching=caching), model_cfg=mc, model=m)
        got, pre = [], []
        for p in prompts:                      # one after the other, so the later ones hit the cache
            del calls[:]
            got.append(eng.generate([p], sp)[0].output)
            assert {w for w, _ in calls} == {40}
            pre.append(calls[0][1])
        outs.append(got)
        first_prefix.append(pre)
    assert outs[0] == outs[1]
    # without the cache every prompt starts at position 0; with it the later prompts start behind a
    # cached prefix, the second behind one longer than the window
    assert first_prefix[0] == [0, 0, 0]
    assert first_prefix[1][0] == 0 and first_prefix[1][1] > 40 and first_prefix[1][2] > 0


def test_eagle3_refuses_a_windowed_target():
    from dgi.engine import EngineConfig
    from dgi.spec.eagle3 import Eagle3Draft, SpecEngine
    mc = dataclasses.replace(get_config("mistral-tiny"), hidden_size=128, intermediate_size=128, num_heads=4,
                             num_kv_heads=2, head_dim=32, vocab_size=512)
    cfg = EngineConfig(model=mc.name, device="cpu", dtype=torch.float32, num_blocks=16, max_num_seqs=2,
                       max_model_len=64, max_num_batched_tokens=32, use_graphs=False)
    with pytest.raises(ValueError, match="sliding-window"):
        SpecEngine(cfg, model_cfg=mc)
    with pytest.raises(ValueError, match="sliding-window"):
        SpecEngine(dataclasses.replace(cfg, model="mistral-tiny"))
    target = LlamaModel(mc, "cpu", torch.float32, seed=1)
    with pytest.raises(ValueError, match="sliding-window"):
        Eagle3Draft(target, 16, 16)
    with pytest.raises(ValueError, match="sliding-window"):
        SpecEngine(cfg, model=target)
    # one windowed layer is enough
    one = dataclasses.replace(mc, window_layers=(1,))
    with pytest.raises(ValueError, match="sliding-window"):
        SpecEngine(cfg, model_cfg=one)


# ---------------------------------------------------------------------------- the GPU tests' checkers

@pytest.mark.parametrize("family", ["count", "needle", "random"])
def test_windowed_checkers_catch_a_one_key_slip(family):
    """tests/swa_cases.py (what test_sliding_window_gpu.py runs the kernels through): the reference
    with the right window passes, one key more or fewer at the window's start fails.  Contexts
    below 64 + W, so no block is poisoned and the CPU reference can read the pool."""
    import swa_cases as sw
    W = 33
    w = sw.build(family, 8, 2, 64, [40, 70, 90], W, device="cpu")
    c = w.c
    run = lambda win: ops.paged_decode_ref(c.q, w.kc, w.vc, c.bt, c.ctx, 8, 2, c.scale, window=win)   # noqa: E731
    assert sw.check(w, run(W)).ok
    for wrong in (W + 1, W - 1, 0):
        assert not sw.check(w, run(wrong)).ok, wrong
    w = sw.build(family, 8, 2, 64, [90, 50], W, [60, 20], device="cpu")
    c = w.c
    run = lambda win: ops.paged_prefill_ref(c.q, w.kc, w.vc, c.bt, c.cu, c.ctx, 8, 2, c.scale, window=win)   # noqa: E731
    assert sw.check(w, run(W)).ok
    for wrong in (W + 1, W - 1, 0):
        assert not sw.check(w, run(wrong)).ok, wrong


def test_windowed_cases_poison_what_the_contract_forbids():
    import swa_cases as sw
    w = sw.build("random", 8, 2, 64, [300], 33, device="cpu")       # lo = 267, lo & ~63 = 256
    c = w.c
    assert c.bt[0, :16].tolist() == [0] * 16 and int(c.bt[0, 16]) != 0
    assert bool(torch.isnan(w.kc[0]).all()) and not bool(torch.isnan(w.kc[c.bt[0, 16].long()]).any())
    p = sw.build("random", 8, 2, 64, [600], 33, [33], device="cpu")  # lo_min = 535, & ~63 = 512
    assert p.c.bt[0, :32].tolist() == [0] * 32 and int(p.c.bt[0, 32]) != 0
