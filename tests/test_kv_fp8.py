"""FP8 KV cache, CPU side: the one quantiser definition, the reference ops on e4m3 pages, an engine with
an fp8 pool (prefix cache, host tier), the layouts that refuse it, the wire format, checkpoint scales
and the public keys (the kernels: test_kv_fp8_gpu.py)."""
import json
import logging
import os

import pytest
import torch

from dgi import ops
from dgi.engine import EngineConfig, LLMEngine, engine_block_budget
from dgi.kv.block_pool import BlockPool, num_blocks_for_budget
from dgi.kv.transfer import pack_kv, unpack_kv
from dgi.models.config import get_config
from dgi.sched.request import SamplingParams

FP8 = torch.float8_e4m3fn
NAME = "llama-tiny-hd128"
PROMPTS = [[1] + list(range(7, 7 + n - 1)) for n in (5, 40, 200, 7)]


def _codes(t):
    return t.view(torch.uint8)


def _pow2(nkv):
    h = torch.arange(nkv)
    return torch.stack([torch.exp2(((h % 5) - 2).float()), torch.exp2((((h + 3) % 5) - 2).float())])


# ----------------------------------------------------------------------------
# quantiser
# ----------------------------------------------------------------------------

def test_quantiser_saturates_instead_of_nan():
    x = torch.tensor([[470.0, 1000.0, -470.0, -1e30, 448.0, 464.0, 3e38, -3e38]])
    q = ops.quantize_kv_ref(x, torch.ones(1))
    assert q.dtype == FP8
    assert q.float().tolist() == [[448.0, 448.0, -448.0, -448.0, 448.0, 448.0, 448.0, -448.0]]
    assert torch.isnan(torch.tensor(470.0).to(FP8).float())          # what the explicit clamp avoids


def test_quantiser_small_values_and_ties():
    sub = 2.0 ** -9                                                   # smallest subnormal
    x = torch.tensor([[sub / 2, -sub / 2, sub * 0.49, sub * 0.51, sub, 1.5 * sub, 2.5 * sub, 0.0]])
    q = ops.quantize_kv_ref(x, torch.ones(1)).float()
    # round to nearest even: a half goes to 0, 1.5 to 2, 2.5 to 2
    assert q.tolist() == [[0.0, -0.0, 0.0, sub, sub, 2 * sub, 2 * sub, 0.0]]


def test_every_finite_code_round_trips():
    b = torch.tensor([x for x in range(256) if x & 0x7F != 0x7F], dtype=torch.uint8)
    assert b.numel() == 254
    vals = b.view(FP8).float()
    assert torch.equal(vals.to(torch.bfloat16).float(), vals)         # exact in bf16: the kernels' widening
    for s in (1.0, 0.25, 4.0, 0.37):
        sc = torch.tensor([s])
        inv = torch.ones(()) / sc
        deq = ops.dequantize_kv_ref(b.view(FP8)[None], sc)
        assert torch.equal(_codes(ops.quantize_kv_ref(deq, inv))[0], b), s


def test_scales_apply_per_kind_and_head():
    nkv, hd = 8, 16
    sc = _pow2(nkv)
    inv = torch.ones(()) / sc
    x = torch.randn(5, nkv, hd).to(torch.bfloat16)
    for j in range(2):
        q = ops.quantize_kv_ref(x, inv[j])
        for h in range(nkv):
            want = torch.clamp(x[:, h].float() * float(inv[j, h]), -448, 448).to(FP8)
            assert torch.equal(_codes(q[:, h]), _codes(want))
        d = ops.dequantize_kv_ref(q, sc[j])
        assert torch.equal(d, q.float() * sc[j][:, None])
    assert not torch.equal(_codes(ops.quantize_kv_ref(x, inv[0])), _codes(ops.quantize_kv_ref(x, inv[1])))


# ----------------------------------------------------------------------------
# reference ops
# ----------------------------------------------------------------------------

def _pool(nblk, nkv, bs, hd, dtype):
    if dtype == FP8:
        return torch.full((2, nblk, nkv, bs, hd), 0x7F, dtype=torch.uint8).view(FP8)
    return torch.full((2, nblk, nkv, bs, hd), float("nan"), dtype=dtype)


@pytest.mark.parametrize("nh,nkv,hd,rd,mode", [(8, 2, 128, 128, 0), (8, 2, 128, 64, 1), (6, 2, 64, 64, 0)])
def test_rope_cache_ref_fp8_is_the_quantised_bf16_write(nh, nkv, hd, rd, mode):
    T, bs, nblk = 37, 16, 5
    g = torch.Generator().manual_seed(1)
    qkv = (torch.randn(T, (nh + 2 * nkv) * hd, generator=g) * 3).to(torch.bfloat16)
    qkv[::5] *= 200.0
    pos = torch.randint(0, 100, (T,), generator=g, dtype=torch.int32)
    slots = torch.randperm(nblk * bs, generator=g)[:T].to(torch.int32)
    slots[::9] = -1
    cs = ops.rope_cos_sin(rd, 128, 10000.0)
    sc = _pow2(nkv) * 1.3
    inv = torch.ones(()) / sc
    kv16, q16 = _pool(nblk, nkv, bs, hd, torch.bfloat16), qkv.clone()
    ops.rope_cache_ref(q16, pos, cs, nh, nkv, hd, slots, kv16[0], kv16[1], mode)
    kv8, q8 = _pool(nblk, nkv, bs, hd, FP8), qkv.clone()
    ops.rope_cache(q8, pos, cs, nh, nkv, hd, slots, kv8[0], kv8[1], mode, kv_inv_scale=inv)
    assert torch.equal(q8.view(torch.int16), q16.view(torch.int16))
    for j in range(2):
        want = ops.quantize_kv_ref(kv16[j].transpose(1, 2), inv[j]).transpose(1, 2)
        assert torch.equal(_codes(kv8[j]), _codes(want.contiguous()))        # NaN (unwritten) -> 0x7F on both sides
    assert int((_codes(kv8) == 0x7F).sum()) == int(torch.isnan(kv16).sum())
    with pytest.raises(ValueError):
        ops.rope_cache(q16, pos, cs, nh, nkv, hd, slots, kv16[0], kv16[1], mode, kv_inv_scale=inv)   # scales, bf16 pages
    with pytest.raises(ValueError):
        ops.rope_cache(q8, pos, cs, nh, nkv, hd, slots, kv8[0], kv8[1], mode, kv_inv_scale=inv[:, :1])


def test_paged_refs_on_codes_equal_the_dequantised_cache():
    nh, nkv, hd, bs, nblk = 8, 2, 64, 16, 12
    g = torch.Generator().manual_seed(2)
    sc = _pow2(nkv)
    kv8 = torch.randint(0, 256, (2, nblk, nkv, bs, hd), generator=g, dtype=torch.uint8)
    kv8[(kv8 & 0x7F) == 0x7F] = 0
    kv8[0] &= 0xBF                                # K: exponent below 8, scores stay finite
    kv8 = kv8.view(FP8)
    deq = torch.stack([ops.dequantize_kv_ref(kv8[j].transpose(1, 2), sc[j]).transpose(1, 2) for j in range(2)])
    deq = deq.to(torch.bfloat16)
    assert torch.equal(deq.float(), torch.stack([kv8[j].float() * sc[j][None, :, None, None] for j in range(2)]))
    ctx = torch.tensor([5, 33, 64], dtype=torch.int32)
    bt = torch.tensor([[1, 0, 0, 0], [2, 3, 4, 0], [5, 6, 7, 8]], dtype=torch.int32)
    q = torch.randn(3, nh * hd, generator=g).to(torch.bfloat16) * 0.1
    a = ops.paged_decode(q, kv8[0], kv8[1], bt, ctx, nh, nkv, 0.125, kv_scale=sc)
    b = ops.paged_decode(q, deq[0], deq[1], bt, ctx, nh, nkv, 0.125)
    assert torch.equal(a, b) and bool(torch.isfinite(a.float()).all())
    qlens = [3, 20, 64]
    cu = torch.tensor([0, 3, 23, 87], dtype=torch.int32)
    qp = torch.randn(sum(qlens), nh * hd, generator=g).to(torch.bfloat16) * 0.1
    a = ops.paged_prefill(qp, kv8[0], kv8[1], bt, cu, ctx, nh, nkv, 0.125, kv_scale=sc)
    b = ops.paged_prefill(qp, deq[0], deq[1], bt, cu, ctx, nh, nkv, 0.125)
    assert torch.equal(a, b)
    # no scales: ones
    a = ops.paged_decode(q, kv8[0], kv8[1], bt, ctx, nh, nkv, 0.125)
    b = ops.paged_decode(q, kv8[0].float().to(torch.bfloat16), kv8[1].float().to(torch.bfloat16), bt, ctx, nh, nkv, 0.125)
    assert torch.equal(a, b)
    with pytest.raises(ValueError):
        ops.paged_decode(q, deq[0], deq[1], bt, ctx, nh, nkv, 0.125, kv_scale=sc)


def test_rope_epilogues_refuse_fp8_pages():
    kv8 = _pool(2, 2, 16, 128, FP8)
    with pytest.raises(ValueError, match="fp8"):
        ops.mfma_gemm_norm_rope(None, None, None, 1e-5, None, None, None, kv8[0], kv8[1], 8, 2)
    with pytest.raises(ValueError, match="fp8"):
        ops.fused_skinny(None, None, None, None, None, 1e-5, None, None, 1, 2, k_cache=kv8[0], v_cache=kv8[1])


# ----------------------------------------------------------------------------
# pool and engine
# ----------------------------------------------------------------------------

def test_block_pool_fp8():
    p16 = BlockPool(8, 16, 2, 2, 128, torch.bfloat16)
    p8 = BlockPool(8, 16, 2, 2, 128, FP8)
    assert p8.kv.dtype == FP8 and p8.is_fp8 and not p16.is_fp8
    assert p8.page_bytes() * 2 == p16.page_bytes()
    assert p16.kv_scale is None and p16.kv_inv_scale is None
    assert tuple(p8.kv_scale.shape) == (2, 2, 2) and bool((p8.kv_scale == 1).all()) and bool((p8.kv_inv_scale == 1).all())
    sc = torch.tensor([[[0.3, 2.0], [1.0, 7.0]], [[0.5, 0.25], [3.0, 1.1]]])
    held = p8.kv_scale
    p8.set_kv_scales(sc)
    assert held is p8.kv_scale and torch.equal(p8.kv_scale, sc)            # in place: views stay valid
    assert torch.equal(p8.kv_inv_scale, torch.ones(()) / sc) and p8.kv_inv_scale.dtype == torch.float32
    for bad in (sc[:1], -sc, sc * float("inf"), torch.zeros_like(sc)):
        with pytest.raises(ValueError):
            p8.set_kv_scales(bad)
    with pytest.raises(ValueError):
        p16.set_kv_scales(sc)
    args = (1 << 30, 32, 8, 128, 16)
    assert num_blocks_for_budget(*args, dtype_bytes=1) == 2 * num_blocks_for_budget(*args)
    src = p8.allocate(1)[0]
    _codes(p8.kv)[:, :, src] = 0x3C
    p8.incref([src])
    new = p8.cow(src)
    assert new != src and bool((_codes(p8.kv)[:, :, new] == 0x3C).all())


def _engine(dtype=torch.float32, **kw):
    base = dict(model=NAME, device="cpu", dtype=dtype, num_blocks=256, max_num_seqs=8, max_model_len=512,
                max_num_batched_tokens=256, use_graphs=False, kv_dtype="fp8")
    base.update(kw)
    return LLMEngine(EngineConfig(**base))


@pytest.fixture(scope="module")
def greedy():
    """Tokens of the fp32 CPU engine with an fp8 pool, prefix cache off: the shared reference."""
    eng = _engine(enable_prefix_caching=False)
    sp = SamplingParams(max_tokens=10, temperature=0.0, ignore_eos=True)
    return eng, [r.output for r in eng.generate(PROMPTS, sp)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_engine_pool_and_budget(dtype):
    eng = _engine(dtype, num_blocks=32)
    ref = _engine(dtype, num_blocks=32, kv_dtype=None)
    assert eng.pool.dtype == FP8 and eng.pool.kv.dtype == FP8 and eng.model.kv_fp8 and not ref.model.kv_fp8
    assert eng.pool.page_bytes() * torch.tensor([], dtype=dtype).element_size() == ref.pool.page_bytes()
    assert eng.model.kv_scale is eng.pool.kv_scale and eng.model.kv_inv_scale is eng.pool.kv_inv_scale
    mc = get_config(NAME)
    auto = dict(model=NAME, device="cpu", dtype=torch.bfloat16, max_num_seqs=100000, max_model_len=512)
    n8 = engine_block_budget(EngineConfig(**auto, kv_dtype="fp8"), mc, mc.num_layers, torch.device("cpu"))
    n16 = engine_block_budget(EngineConfig(**auto), mc, mc.num_layers, torch.device("cpu"))
    assert n8 == 2 * n16
    out = eng.generate([PROMPTS[1]], SamplingParams(max_tokens=4, temperature=0.0, ignore_eos=True))[0].output
    assert len(out) == 4
    written = _codes(eng.pool.kv)
    assert bool((written != 0).any())


def test_engine_prefix_cache_gives_the_same_tokens(greedy):
    _, want = greedy
    eng = _engine(enable_prefix_caching=True)
    sp = SamplingParams(max_tokens=10, temperature=0.0, ignore_eos=True)
    first = [r.output for r in eng.generate(PROMPTS, sp)]
    again = [r.output for r in eng.generate(PROMPTS, sp)]           # now served from cached e4m3 pages
    assert first == want and again == want
    assert eng.scheduler.radix.hits_tokens >= 192                   # the 200-token prompt's 12 full pages


def test_engine_host_tier_spill_and_restore():
    base = dict(model=NAME, device="cpu", dtype=torch.float32, max_num_seqs=6, max_num_batched_tokens=256,
                max_model_len=256, use_graphs=False, enable_prefix_caching=False, kv_dtype="fp8")
    g = torch.Generator().manual_seed(3)
    prompts = [torch.randint(5, 500, (20 + 3 * i,), generator=g).tolist() for i in range(6)]
    sp = SamplingParams(max_tokens=24, temperature=0.0, ignore_eos=True)
    big = LLMEngine(EngineConfig(**base, num_blocks=256))
    want = [r.output for r in big.generate(prompts, sp)]
    eng = LLMEngine(EngineConfig(**base, num_blocks=17, host_kv_gb=0.05), model=big.model)
    got = [r.output for r in eng.generate(prompts, sp)]
    st = eng.scheduler.stats()
    assert eng.host_tier.host.dtype == FP8
    assert got == want
    assert st["preemptions"] > 0 and st["swapped_out"] == st["preemptions"] == st["swapped_in"]
    assert eng.stats["prefill_tokens"] == sum(len(p) for p in prompts)


def test_engine_config_rejects_unknown_kv_dtype():
    with pytest.raises(ValueError, match="kv_dtype"):
        EngineConfig(model=NAME, device="cpu", kv_dtype="int8")
    assert EngineConfig(model=NAME, device="cpu").kv_dtype is None


def test_bf16_cpu_engine_stays_inside_the_gpu_tolerance(greedy):
    """The check the GPU engine test relies on (rel 0.03, abs 0.02 of test_fp8_weights_gpu): a bf16 CPU
    engine with an fp8 pool, teacher forced against the fp32 CPU engine with the same pool."""
    from dgi.models.llama import LlamaModel
    ref, _ = greedy
    mc = get_config(NAME)
    bm = LlamaModel(mc, "cpu", torch.bfloat16, init="empty").copy_from(ref.model)
    beng = LLMEngine(EngineConfig(model=NAME, device="cpu", dtype=torch.bfloat16, num_blocks=256, max_num_seqs=8,
                                  max_model_len=512, max_num_batched_tokens=256, use_graphs=False, kv_dtype="fp8",
                                  enable_prefix_caching=False), model_cfg=mc, model=bm)
    sp = SamplingParams(max_tokens=10, temperature=0.0, ignore_eos=True)
    outs = [r.output for r in beng.generate(PROMPTS, sp)]
    got = {}
    orig = ref.model.compute_logits

    def spy(h, residual, idx):
        out = orig(h, residual, idx)
        got["l"] = out[-1].detach().float()
        return out
    ref.model.compute_logits = spy
    one = SamplingParams(max_tokens=1, temperature=0.0, ignore_eos=True)
    worst = 0.0
    try:
        for p, toks in zip(PROMPTS, outs):
            for t, tok in enumerate(toks):
                ref.generate([p + toks[:t]], one)
                r = got["l"]
                tol = 0.03 * float(r.abs().max()) + 0.02
                gap = float(r.max()) - float(r[tok])
                worst = max(worst, gap / tol)
                assert gap <= tol, (len(p), t, tok, int(r.argmax()), gap, tol)
    finally:
        ref.model.compute_logits = orig
    print(f"KVFP8 bf16-vs-fp32 CPU pair: worst gap / tolerance = {worst:.4f}")


# ----------------------------------------------------------------------------
# refusals
# ----------------------------------------------------------------------------

def _cfg(**kw):
    return EngineConfig(model=NAME, device="cpu", dtype=torch.float32, num_blocks=32, max_num_seqs=4,
                        max_model_len=128, use_graphs=False, kv_dtype="fp8", **kw)


def test_layouts_that_refuse_an_fp8_pool():
    from dgi.parallel.pd import DecodeDriver, PrefillServer
    from dgi.parallel.pipeline import PipelineEngine, StageWorker
    from dgi.parallel.tensor import TPEngine
    from dgi.spec.eagle3 import SpecEngine
    cfg = _cfg()
    with pytest.raises(ValueError, match="pipeline"):
        PipelineEngine(cfg, None, [0, 1])
    with pytest.raises(ValueError, match="pipeline"):
        StageWorker(cfg, None, [0, 1])
    with pytest.raises(ValueError, match="disaggregation"):
        PrefillServer(cfg, None, None)
    with pytest.raises(ValueError, match="disaggregation"):
        DecodeDriver(cfg, None, None)
    with pytest.raises(ValueError, match="tensor parallel"):
        TPEngine(cfg, 0, 2)
    with pytest.raises(ValueError, match="EAGLE"):
        SpecEngine(cfg)
    with pytest.raises(ValueError, match="pipeline"):
        LLMEngine(_cfg(layer_start=0, layer_end=1))          # a bare partial layer range is a pipeline stage


def test_import_prefilled_refuses_other_dtypes_and_scales():
    donor = _engine(enable_prefix_caching=False, num_blocks=64)
    got = []
    donor.first_token_hook = lambda r: got.append((donor.export_request_kv(r), r.output[0]))
    sp = SamplingParams(max_tokens=6, temperature=0.0, ignore_eos=True)
    want = donor.generate([PROMPTS[1]], sp)[0].output
    (kv, first), = got
    assert kv.dtype == FP8
    blob = pack_kv(kv, {"prompt": PROMPTS[1], "first_token": first}, kv_scale=donor.pool.kv_scale)
    kv2, meta = unpack_kv(blob)
    assert kv2.dtype == FP8 and torch.equal(_codes(kv2), _codes(kv))
    assert meta["kv_scale"].dtype == torch.float32 and torch.equal(meta["kv_scale"], donor.pool.kv_scale)
    taker = LLMEngine(EngineConfig(**{**donor.cfg.__dict__}), model=donor.model)
    r = taker.import_prefilled(meta["prompt"], meta["first_token"], kv2, sp, kv_scale=meta["kv_scale"])
    while taker.has_unfinished():
        taker.step()
    assert r.output == want
    with pytest.raises(ValueError, match="scales"):
        taker.import_prefilled(meta["prompt"], first, kv2, sp)                              # no scales
    with pytest.raises(ValueError, match="scales"):
        taker.import_prefilled(meta["prompt"], first, kv2, sp, kv_scale=meta["kv_scale"] * 2)
    with pytest.raises(ValueError, match="dtype"):
        taker.import_prefilled(meta["prompt"], first, kv2.float().to(torch.bfloat16), sp, kv_scale=meta["kv_scale"])
    plain = LLMEngine(EngineConfig(**{**donor.cfg.__dict__, "kv_dtype": None}), model=donor.model)
    with pytest.raises(ValueError, match="dtype"):
        plain.import_prefilled(meta["prompt"], first, kv2, sp, kv_scale=meta["kv_scale"])
    assert taker.pool.num_free == taker.pool.num_blocks - 1 and plain.pool.num_free == plain.pool.num_blocks - 1


def test_pack_kv_round_trips_fp8_pages_bit_for_bit():
    g = torch.Generator().manual_seed(4)
    raw = torch.randint(0, 256, (2, 2, 3, 2, 16, 64), generator=g, dtype=torch.uint8)
    sc = torch.rand(2, 2, 2, generator=g) + 0.1
    t, meta = unpack_kv(pack_kv(raw.view(FP8), {"prompt": [1, 2, 3], "first_token": 7}, kv_scale=sc))
    assert t.dtype == FP8 and torch.equal(_codes(t), raw)                  # NaN codes included
    assert torch.equal(meta["kv_scale"], sc) and meta["prompt"] == [1, 2, 3] and meta["first_token"] == 7
    with pytest.raises(ValueError):
        pack_kv(raw.view(FP8), {})
    with pytest.raises(ValueError):
        pack_kv(torch.zeros(1, 2, 1, 1, 16, 64, dtype=torch.bfloat16), {}, kv_scale=sc)
    t16, m16 = unpack_kv(pack_kv(torch.ones(1, 2, 1, 1, 16, 64, dtype=torch.bfloat16), {"a": 1}))
    assert t16.dtype == torch.bfloat16 and "kv_scale" not in m16


# ----------------------------------------------------------------------------
# checkpoint scales
# ----------------------------------------------------------------------------

def _write_checkpoint(path, with_scales):
    from safetensors.torch import save_file
    from dgi.models.llama import LlamaModel
    mc = get_config("llama-tiny")
    m = LlamaModel(mc, "cpu", torch.float32, seed=3)
    hd, nh, nkv = mc.head_dim, mc.num_heads, mc.num_kv_heads
    t = {"model.embed_tokens.weight": m.embed, "model.norm.weight": m.norm}
    if m.lm_head is not m.embed:
        t["lm_head.weight"] = m.lm_head
    for i, L in enumerate(m.layers):
        p = f"model.layers.{i}."
        ql, kl = nh * hd, nkv * hd
        t[p + "self_attn.q_proj.weight"] = L.qkv[:ql]
        t[p + "self_attn.k_proj.weight"] = L.qkv[ql:ql + kl]
        t[p + "self_attn.v_proj.weight"] = L.qkv[ql + kl:]
        t[p + "self_attn.o_proj.weight"] = L.o
        I = L.gate_up.shape[0] // 2
        t[p + "mlp.gate_proj.weight"] = L.gate_up[:I]
        t[p + "mlp.up_proj.weight"] = L.gate_up[I:]
        t[p + "mlp.down_proj.weight"] = L.down
        t[p + "input_layernorm.weight"] = L.in_norm
        t[p + "post_attention_layernorm.weight"] = L.post_norm
        if with_scales:
            t[p + "self_attn.k_scale"] = torch.tensor(0.5 + i)
            if i != 1:                      # layer 1 has no v_scale: it keeps 1.0
                t[p + "self_attn.v_scale"] = torch.tensor([0.125 * (i + 1)])
    os.makedirs(path, exist_ok=True)
    save_file({k: v.detach().clone().contiguous() for k, v in t.items()}, os.path.join(path, "model.safetensors"))
    hf = {"architectures": ["LlamaForCausalLM"], "model_type": "llama", "hidden_size": mc.hidden_size,
          "intermediate_size": mc.intermediate_size, "num_hidden_layers": mc.num_layers,
          "num_attention_heads": nh, "num_key_value_heads": nkv, "head_dim": hd, "vocab_size": mc.vocab_size,
          "rms_norm_eps": mc.rms_eps, "rope_theta": mc.rope_theta, "max_position_embeddings": mc.max_position,
          "tie_word_embeddings": m.lm_head is m.embed, "eos_token_id": mc.eos_token_id}
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(hf, f)
    return mc


@pytest.mark.parametrize("with_scales", [True, False])
def test_checkpoint_kv_scales(tmp_path, with_scales, caplog):
    pytest.importorskip("safetensors")
    mc = _write_checkpoint(str(tmp_path / "ckpt"), with_scales)
    with caplog.at_level(logging.INFO):
        eng = LLMEngine(EngineConfig(model=str(tmp_path / "ckpt"), device="cpu", dtype=torch.float32, num_blocks=32,
                                     max_num_seqs=2, max_model_len=128, use_graphs=False, kv_dtype="fp8"))
    sc = eng.pool.kv_scale
    assert tuple(sc.shape) == (mc.num_layers, 2, mc.num_kv_heads)
    if with_scales:
        for i in range(mc.num_layers):
            assert bool((sc[i, 0] == 0.5 + i).all())
            assert bool((sc[i, 1] == (1.0 if i == 1 else 0.125 * (i + 1))).all())
        assert torch.equal(eng.pool.kv_inv_scale, torch.ones(()) / sc)
    else:
        assert bool((sc == 1).all())
        lines = [r for r in caplog.records if "k_scale" in r.getMessage() and "ones" in r.getMessage()]
        assert len(lines) == 1
    out = eng.generate([[1, 5, 9, 13]], SamplingParams(max_tokens=3, temperature=0.0, ignore_eos=True))[0].output
    assert len(out) == 3


# ----------------------------------------------------------------------------
# public keys
# ----------------------------------------------------------------------------

@pytest.mark.parametrize("key,value,expect", [("kv_cache_dtype", "fp8", "fp8"), ("kv_dtype", "fp8", "fp8"),
                                              ("kv_cache_dtype", "auto", None), ("kv_cache_dtype", "int8", None)])
def test_native_worker_kv_cache_dtype_key(key, value, expect, caplog):
    from engines.llm_native import NativeLLMEngine
    e = NativeLLMEngine({"model_id": "llama-tiny", "device": "cpu", "max_model_len": 256, "num_blocks": 64,
                         "max_num_seqs": 4, key: value})
    with caplog.at_level(logging.WARNING, logger="engines.llm_native"):
        e.load_model()
    try:
        assert e.engine.cfg.kv_dtype == expect
        assert e.engine.pool.dtype == (FP8 if expect else e.engine.cfg.dtype)
        warned = [r for r in caplog.records if "kv_cache_dtype" in r.getMessage()]
        assert bool(warned) == (value == "int8")
    finally:
        e.unload_model()


def test_node_flag_reaches_engine_config():
    from dgi.serve import node
    seen = {}

    class Stop(Exception):
        pass

    def fake_router(args, fabric, layout):
        seen["kv"] = args.kv_dtype
        raise Stop
    orig, node.Router = node.Router, fake_router
    try:
        for argv, want in ((["--kv-dtype", "fp8"], "fp8"), ([], None)):
            with pytest.raises(Stop):
                node.main(argv)
            assert seen["kv"] == want
        with pytest.raises(SystemExit):
            node.main(["--kv-dtype", "int8"])
    finally:
        node.Router = orig
