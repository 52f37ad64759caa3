"""Qwen3 on the GPU: the q/k-norm + RoPE + paged-KV writer against its definition
(``ops.qknorm_rope_cache_ref``), bf16 and e4m3 pages, and the engine on ``qwen3-tiny`` and on a
Hugging Face ``Qwen3ForCausalLM`` checkpoint (the CPU side: tests/test_qwen3.py)."""
import pytest
import torch

from dgi import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP8 = torch.float8_e4m3fn
NAN_CODE = 0x7F
POISON16 = 0x7F7F           # a bf16 NaN pattern no kernel writes
EPS = 1e-6


@pytest.fixture(autouse=True, scope="module")
def _native():
    ops.load_native(required=True)


# ----------------------------------------------------------------------------
# kernel
# ----------------------------------------------------------------------------

GEOMS = [(5, 1, 128), (14, 2, 64), (32, 8, 128), (64, 8, 128)]
ROWS = [1, 7, 300]
BS = 16


def _case(nh, nkv, hd, T, seed=0):
    """Inputs in the manner of test_kv_fp8_gpu._writer_case: random positions, permuted slots with
    about a tenth set to -1.  Gains are uniform in [0.25, 4] and differ between q and k; every head's
    input carries its own power-of-two scale (2^-10 .. 2^5, so eps decides the smallest heads): a norm
    over the wrong span or with the other gain is off by a factor, not by a rounding.

    The magnitudes are (1 + u) * 2^k with u in [0, 1): the squares of such bf16 values are multiples
    of 2^(2k - 14) below 2^(2k + 2), so every partial sum of up to 128 of them fits fp32's 24 bits
    and the mean square is exact in ANY summation order.  The comparison then does not depend on the
    order in which the reference's BLAS-free reduction happens to add, and a reduction carried out in
    less than fp32 shows up as a different head scale."""
    g = torch.Generator().manual_seed(1000 * seed + 10 * T + nh)
    nblk = (T + BS - 1) // BS + 3
    heads = nh + 2 * nkv
    mag = 1.0 + torch.rand(T, heads, hd, generator=g)
    sign = torch.where(torch.rand(T, heads, hd, generator=g) < 0.5, -1.0, 1.0)
    scale = torch.exp2(((torch.arange(heads) * 7) % 16 - 10).float())
    qkv = (mag * sign).to(torch.bfloat16) * scale[None, :, None].to(torch.bfloat16)
    qkv = qkv.reshape(T, heads * hd).contiguous()
    pos = torch.randint(0, 500, (T,), generator=g, dtype=torch.int32)
    slots = torch.randperm(nblk * BS, generator=g)[:T].to(torch.int32)
    slots[torch.rand(T, generator=g) < 0.1] = -1
    cos_sin = ops.rope_cos_sin(hd, 512, 1000000.0)
    q_gain = (0.25 + 3.75 * torch.rand(hd, generator=g)).to(torch.bfloat16)
    k_gain = (0.25 + 3.75 * torch.rand(hd, generator=g)).to(torch.bfloat16)
    return qkv, pos, cos_sin, slots, nblk, q_gain, k_gain


def _pages16(nblk, nkv, hd, dev):
    return torch.full((2, nblk, nkv, BS, hd), POISON16, dtype=torch.int16, device=dev).view(torch.bfloat16)


def _pages8(nblk, nkv, hd, dev):
    return torch.full((2, nblk, nkv, BS, hd), NAN_CODE, dtype=torch.uint8, device=dev).view(FP8)


def _per_slot(pages):
    """[nblk, nkv, bs, hd] -> [nblk * bs, nkv, hd]"""
    return pages.permute(0, 2, 1, 3).reshape(-1, pages.shape[1], pages.shape[3])


_REF = {}


def _reference(nh, nkv, hd, T):
    """The definition on the CPU, computed once per case and shared (never modified)."""
    key = (nh, nkv, hd, T)
    if key not in _REF:
        qkv, pos, cs, slots, nblk, qg, kg = _case(nh, nkv, hd, T)
        q, kv = qkv.clone(), _pages16(nblk, nkv, hd, "cpu")
        ops.qknorm_rope_cache_ref(q, pos, cs, qg, kg, EPS, nh, nkv, hd, slots, kv[0], kv[1])
        _REF[key] = (q, kv)
    return _REF[key]


def _run_gpu(nh, nkv, hd, T, fp8, inv=None):
    qkv, pos, cs, slots, nblk, qg, kg = _case(nh, nkv, hd, T)
    q = qkv.to(DEV)
    kv = (_pages8 if fp8 else _pages16)(nblk, nkv, hd, DEV)
    ops.qknorm_rope_cache(q, pos.to(DEV), cs.to(DEV), qg.to(DEV), kg.to(DEV), EPS, nh, nkv, hd, slots.to(DEV),
                          kv[0], kv[1], kv_inv_scale=None if inv is None else inv.to(DEV))
    torch.cuda.synchronize()
    return q.cpu(), kv.cpu(), slots, qkv


@pytest.mark.parametrize("T", ROWS)
@pytest.mark.parametrize("nh,nkv,hd", GEOMS)
def test_qknorm_rope_cache_bf16_pages(nh, nkv, hd, T):
    want_q, want_kv = _reference(nh, nkv, hd, T)
    got_q, got_kv, slots, qkv = _run_gpu(nh, nkv, hd, T, fp8=False)
    nq, nk = nh * hd, nkv * hd
    written = torch.zeros(got_kv.shape[1] * BS, dtype=torch.bool)
    written[slots[slots >= 0].long()] = True
    gk, wk = _per_slot(got_kv[0]), _per_slot(want_kv[0])
    dq = (got_q[:, :nq].float() - want_q[:, :nq].float()).abs().max()
    dk = (gk[written].float() - wk[written].float()).abs().max() if written.any() else 0.0
    print(f"nh={nh} nkv={nkv} hd={hd} T={T}: max |dq| {float(dq):.4g}, max |dk| {float(dk):.4g}, "
          f"max |q| {float(want_q[:, :nq].float().abs().max()):.4g}")
    torch.testing.assert_close(got_q[:, :nq].float(), want_q[:, :nq].float(), atol=2e-2, rtol=2e-2)
    torch.testing.assert_close(gk[written].float(), wk[written].float(), atol=2e-2, rtol=2e-2)
    # the k and v columns of the row are left alone, v pages and every unwritten slot are bit-exact
    assert torch.equal(got_q[:, nq:].view(torch.int16), qkv[:, nq:].view(torch.int16))
    gv, wv = _per_slot(got_kv[1]).view(torch.int16), _per_slot(want_kv[1]).view(torch.int16)
    assert torch.equal(gv, wv)
    live = slots >= 0
    assert torch.equal(gv[written], qkv[:, nq + nk:].reshape(T, nkv, hd)[live][
        torch.argsort(slots[live])].view(torch.int16))
    assert bool((gv[~written] == POISON16).all())
    assert bool((gk.view(torch.int16)[~written] == POISON16).all())
    assert torch.equal(gk.view(torch.int16)[~written], wk.view(torch.int16)[~written])
    assert not bool(torch.isnan(gk[written].float()).any())


@pytest.mark.parametrize("T", ROWS)
@pytest.mark.parametrize("nh,nkv,hd", GEOMS)
def test_qknorm_rope_cache_fp8_pages_are_the_quantised_bf16_pages(nh, nkv, hd, T):
    """The e4m3 instantiation does the bf16 one's arithmetic: its codes are ``quantize_kv_ref`` of
    the pages the bf16 call wrote from the same inputs, bit for bit, and q is the same."""
    h = torch.arange(nkv)
    scale = torch.stack([torch.exp2(((h % 5) - 2).float()), torch.exp2((((h + 3) % 5) - 2).float())])
    inv = torch.ones((), dtype=torch.float32) / scale
    q16, kv16, slots, _ = _run_gpu(nh, nkv, hd, T, fp8=False)
    q8, kv8, _, _ = _run_gpu(nh, nkv, hd, T, fp8=True, inv=inv)
    assert torch.equal(q8.view(torch.int16), q16.view(torch.int16))
    written = torch.zeros(kv16.shape[1] * BS, dtype=torch.bool)
    written[slots[slots >= 0].long()] = True
    for j in (0, 1):
        got = _per_slot(kv8[j]).view(torch.uint8)
        want = ops.quantize_kv_ref(_per_slot(kv16[j])[written], inv[j]).view(torch.uint8)
        assert torch.equal(got[written], want), f"{'kv'[j]}: {int((got[written] != want).sum())} codes differ"
        assert bool((got[~written] == NAN_CODE).all())
        assert not bool(((got[written] & 0x7F) == NAN_CODE).any())


@pytest.mark.parametrize("nh,nkv,hd", [(5, 1, 128), (14, 2, 64)])
def test_qknorm_rope_cache_general_inputs(nh, nkv, hd):
    """Values as test_kv_fp8_gpu._writer_case draws them (N(0, 1), a tenth of the entries around 2000
    and a tenth around 2^-14), times a power of two per head: the sums of squares are not exact here,
    so the kernel's mean square may differ from the reference's in its last bits (another summation
    order), and where the fp32 product sits on a bf16 rounding boundary the normalised value n then
    rounds the other way — one bf16 ulp, at most 2^-7 |n|.  The rotation carries that into the output
    with weights |cos|, |sin| <= 1.  Bound: the 2e-2 / 2e-2 of the exact-sum cases plus
    2^-7 (|n[d]| + |n[partner of d]|); a wrong gain, span or eps is off by a factor."""
    T = 300
    g = torch.Generator().manual_seed(7)
    heads = nh + 2 * nkv
    nblk = (T + BS - 1) // BS + 3
    x = torch.randn(T, heads, hd, generator=g)
    u = torch.rand(T, heads, hd, generator=g)
    x = torch.where(u < 0.1, x * 2000.0, torch.where(u > 0.9, x * 2.0 ** -14, x))
    x = x * torch.exp2(((torch.arange(heads) * 5) % 12 - 8).float())[None, :, None]
    qkv = x.to(torch.bfloat16).reshape(T, heads * hd)
    pos = torch.randint(0, 500, (T,), generator=g, dtype=torch.int32)
    slots = torch.randperm(nblk * BS, generator=g)[:T].to(torch.int32)
    slots[torch.rand(T, generator=g) < 0.1] = -1
    cs = ops.rope_cos_sin(hd, 512, 1000000.0)
    qg = (0.25 + 3.75 * torch.rand(hd, generator=g)).to(torch.bfloat16)
    kg = (0.25 + 3.75 * torch.rand(hd, generator=g)).to(torch.bfloat16)
    want_q, want_kv = qkv.clone(), _pages16(nblk, nkv, hd, "cpu")
    ops.qknorm_rope_cache_ref(want_q, pos, cs, qg, kg, EPS, nh, nkv, hd, slots, want_kv[0], want_kv[1])
    got_q, got_kv = qkv.to(DEV), _pages16(nblk, nkv, hd, DEV)
    ops.qknorm_rope_cache(got_q, pos.to(DEV), cs.to(DEV), qg.to(DEV), kg.to(DEV), EPS, nh, nkv, hd, slots.to(DEV),
                          got_kv[0], got_kv[1])
    torch.cuda.synchronize()
    got_q, got_kv = got_q.cpu(), got_kv.cpu()
    live = slots >= 0
    rows = slots[live].long()
    nq, nk = nh * hd, nkv * hd
    worst = 0.0
    for name, got, want, raw, gain in (
            ("q", got_q[:, :nq].view(T, nh, hd), want_q[:, :nq].view(T, nh, hd), qkv[:, :nq].view(T, nh, hd), qg),
            ("k", _per_slot(got_kv[0])[rows], _per_slot(want_kv[0])[rows],
             qkv[:, nq:nq + nk].reshape(T, nkv, hd)[live], kg)):
        n = ops.rmsnorm_ref(raw, gain, EPS).float().abs()
        bound = 2e-2 + 2e-2 * want.float().abs() + 2.0 ** -7 * (n + n.roll(hd // 2, -1))
        err = (got.float() - want.float()).abs()
        worst = max(worst, float((err / bound).max()))
        print(f"{name}: max err {float(err.max()):.4g}, max err / bound {float((err / bound).max()):.3f}, "
              f"elements off {int((err > 0).sum())} of {err.numel()}")
        assert bool((err <= bound).all()), (name, float((err / bound).max()))
    assert torch.equal(got_kv[1].view(torch.int16), want_kv[1].view(torch.int16))
    written = torch.zeros(nblk * BS, dtype=torch.bool)
    written[rows] = True
    assert bool((_per_slot(got_kv[0]).view(torch.int16)[~written] == POISON16).all())


def test_qknorm_rope_cache_refusals():
    nh, nkv = 8, 2

    def operands(hd, rd=None):
        qkv = torch.zeros(4, (nh + 2 * nkv) * hd, dtype=torch.bfloat16, device=DEV)
        pos = torch.zeros(4, dtype=torch.int32, device=DEV)
        cs = ops.rope_cos_sin(rd or hd, 16, 10000.0, device=DEV)
        gain = torch.ones(hd, dtype=torch.bfloat16, device=DEV)
        kv16 = torch.zeros(2, 2, nkv, 16, hd, dtype=torch.bfloat16, device=DEV)
        kv8 = torch.zeros(2, 2, nkv, 16, hd, dtype=torch.uint8, device=DEV).view(FP8)
        return qkv, pos, cs, gain, kv16, kv8
    call = torch.ops.dgi.qknorm_rope_cache
    qkv, pos, cs, g, kv16, kv8 = operands(128)
    call(qkv, pos, cs, g, g, EPS, nh, nkv, 128, pos, kv16[0], kv16[1], None)          # the accepted form
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):       # gains of the wrong length
        call(qkv, pos, cs, g[:64], g, EPS, nh, nkv, 128, pos, kv16[0], kv16[1], None)
    with pytest.raises(RuntimeError):
        call(qkv, pos, cs, g, torch.ones(256, dtype=torch.bfloat16, device=DEV), EPS, nh, nkv, 128, pos,
             kv16[0], kv16[1], None)
    with pytest.raises(RuntimeError):       # gains of the wrong dtype
        call(qkv, pos, cs, g.float(), g, EPS, nh, nkv, 128, pos, kv16[0], kv16[1], None)
    with pytest.raises(RuntimeError):       # gains on the host
        call(qkv, pos, cs, g, g.cpu(), EPS, nh, nkv, 128, pos, kv16[0], kv16[1], None)
    with pytest.raises(RuntimeError):       # an fp8 cache without scales
        call(qkv, pos, cs, g, g, EPS, nh, nkv, 128, pos, kv8[0], kv8[1], None)
    with pytest.raises(RuntimeError):       # scales with bf16 pages
        call(qkv, pos, cs, g, g, EPS, nh, nkv, 128, pos, kv16[0], kv16[1], torch.ones(2, nkv, device=DEV))
    with pytest.raises(RuntimeError):       # partial rotary: a [max_pos, 64] table for 128-dim heads
        call(qkv, pos, operands(128, 64)[2], g, g, EPS, nh, nkv, 128, pos, kv16[0], kv16[1], None)
    with pytest.raises(ValueError):         # interleaved pairing
        ops.qknorm_rope_cache(qkv, pos, cs, g, g, EPS, nh, nkv, 128, pos, kv16[0], kv16[1], mode=1)
    qkv, pos, cs, g, kv16, _ = operands(96)
    with pytest.raises(RuntimeError):       # head_dim 96
        call(qkv, pos, cs, g, g, EPS, nh, nkv, 96, pos, kv16[0], kv16[1], None)


def test_model_refuses_a_geometry_the_kernel_does_not_take():
    from dgi.models.config import ModelConfig
    from dgi.models.llama import LlamaModel
    base = dict(name="t", arch="qwen3", vocab_size=64, hidden_size=256, intermediate_size=256, num_layers=1,
                num_heads=2, num_kv_heads=1, max_position=64, qk_norm=True)
    for kw in (dict(head_dim=96), dict(head_dim=128, rotary_dim=64), dict(head_dim=128, rope_interleaved=True)):
        with pytest.raises(ValueError):
            LlamaModel(ModelConfig(**base, **kw), DEV)
        LlamaModel(ModelConfig(**base, **kw), "cpu")        # the reference path takes them all


# ----------------------------------------------------------------------------
# engine
# ----------------------------------------------------------------------------

def _count_op(monkeypatch):
    calls = []
    orig = ops.qknorm_rope_cache

    def counted(*a, **k):
        calls.append(a[0].shape[0])
        return orig(*a, **k)
    monkeypatch.setattr(ops, "qknorm_rope_cache", counted)
    return calls


def _teacher_forced_ok(name, src_model, prompts, gpu_outs, rel=0.03, abs_=0.02, kv_dtype=None):
    """tests/test_kernels_gpu._teacher_forced_ok: every token the GPU chose is an argmax of the fp32
    CPU model's logits for the same prefix (teacher forced), up to a bf16 tolerance — per step, every
    prompt.  ``kv_dtype="fp8"``: the reference engine on an fp8 pool, as tests/test_kv_fp8_gpu has it."""
    from dgi.engine import EngineConfig, LLMEngine
    from dgi.models.llama import LlamaModel
    from dgi.sched.request import SamplingParams
    mc = src_model.cfg
    f32 = LlamaModel(mc, "cpu", torch.float32, init="empty").copy_from(src_model)
    kw = {"kv_dtype": kv_dtype} if kv_dtype else {}
    # 512 tokens per step: the oracle prefills every prompt here (up to 309 tokens) in one chunk, so
    # each generate() below computes exactly one row of logits
    ref = LLMEngine(EngineConfig(model=name, device="cpu", dtype=torch.float32, num_blocks=256, max_num_seqs=8,
                                 max_model_len=512, max_num_batched_tokens=512, use_graphs=False,
                                 enable_prefix_caching=False, **kw), model_cfg=mc, model=f32)
    got = {}
    orig = ref.model.compute_logits

    def spy(h, residual, idx):
        out = orig(h, residual, idx)
        got["l"] = out[-1].detach().float()
        return out
    ref.model.compute_logits = spy
    one = SamplingParams(max_tokens=1, temperature=0.0, ignore_eos=True)
    checked = 0
    worst = 0.0
    for p, toks in zip(prompts, gpu_outs):
        for t, tok in enumerate(toks):
            ref.generate([p + toks[:t]], one)
            r = got["l"]
            tol = rel * float(r.abs().max()) + abs_
            worst = max(worst, (float(r.max()) - float(r[tok])) / tol)
            assert float(r[tok]) >= float(r.max()) - tol, (name, len(p), t, tok, int(r.argmax()))
            checked += 1
    print(f"{name} kv={kv_dtype}: {checked} tokens, worst (max - chosen) / tol = {worst:.3f}")
    return checked


def test_qwen3_engine_gpu_matches_cpu(monkeypatch):
    """qwen3-tiny (q_size = 2 * hidden) through the native kernels against the fp32 CPU engine.  The
    300-token prompt's step runs the fused-norm layers (forced: a test-size model has no routing
    table, so the default would keep them off) and the decode steps the fused decode layers, both
    with the plain qkv epilogue followed by the q/k-norm writer."""
    from dgi.engine import EngineConfig, LLMEngine
    from dgi.models import llama
    from dgi.models.config import get_config
    from dgi.models.llama import LlamaModel
    from dgi.sched.request import SamplingParams
    monkeypatch.setattr(llama, "NORM_FOLD", "force")
    mc = get_config("qwen3-tiny")
    cpu_model = LlamaModel(mc, "cpu", seed=5)
    prompts = [[1] + list(range(7, 7 + n - 1)) for n in (3, 60, 300)]
    sp = SamplingParams(max_tokens=10, temperature=0.0, ignore_eos=True)
    gm = LlamaModel(mc, "cuda", init="empty").copy_from(cpu_model)
    paths = {"folded": 0, "fused": 0}
    for key, name in (("folded", "_forward_layers_folded"), ("fused", "_forward_layers_fused")):
        def spy(*a, _k=key, _o=getattr(gm, name), **k):
            paths[_k] += 1
            return _o(*a, **k)
        setattr(gm, name, spy)
    calls = _count_op(monkeypatch)
    ge = LLMEngine(EngineConfig(model="qwen3-tiny", device="cuda", num_blocks=128, max_num_seqs=4, max_model_len=512,
                                max_num_batched_tokens=512, use_graphs=True), model_cfg=mc, model=gm)
    gpu = [r.output for r in ge.generate(prompts, sp)]
    torch.cuda.synchronize()
    assert len(calls) >= mc.num_layers and max(calls) >= 300
    assert paths["folded"] > 0 and paths["fused"] > 0, paths
    assert _teacher_forced_ok("qwen3-tiny", cpu_model, prompts, gpu) == 30


def test_qwen3_engine_fp8_kv(monkeypatch):
    """One run on e4m3 pages, held to the bound of test_kv_fp8_gpu.test_fp8_kv_engine_teacher_forced
    (its prompts, 10 tokens each, the fp32 reference engine on an fp8 pool, 0.03 * max|ref| + 0.02)."""
    from dgi.engine import EngineConfig, LLMEngine
    from dgi.models.config import get_config
    from dgi.models.llama import LlamaModel
    from dgi.sched.request import SamplingParams
    name = "qwen3-tiny"
    mc = get_config(name)
    src = LlamaModel(mc, "cpu", seed=5)
    prompts = [[1] + list(range(7, 7 + n - 1)) for n in (5, 40, 200, 7)]
    sp = SamplingParams(max_tokens=10, temperature=0.0, ignore_eos=True)
    gm = LlamaModel(mc, "cuda", init="empty").copy_from(src)
    calls = _count_op(monkeypatch)
    eng = LLMEngine(EngineConfig(model=name, device="cuda", num_blocks=256, max_num_seqs=8, max_model_len=512,
                                 max_num_batched_tokens=256, use_graphs=True, kv_dtype="fp8"), model_cfg=mc, model=gm)
    assert eng.pool.dtype == FP8 and gm.kv_fp8
    outs = [r.output for r in eng.generate(prompts, sp)]
    torch.cuda.synchronize()
    assert calls and all(len(o) == 10 for o in outs)
    assert _teacher_forced_ok(name, src, prompts, outs, kv_dtype="fp8") == 40


# ----------------------------------------------------------------------------
# Hugging Face parity (bf16 on the GPU against HF fp32)
# ----------------------------------------------------------------------------

H, I, L, NH, NKV, HD, V = 512, 1024, 2, 8, 2, 128, 1024            # q_size = 1024 != hidden
HF_PROMPTS = [[1, 33, 44, 55, 66, 77, 88, 99, 111, 222], [1] + list(range(300, 300 + 140))]


def _tol(ref):
    return 0.03 * float(ref.abs().max()) + 0.02


def test_gpu_bf16_per_step_logits_match_hf(tmp_path, monkeypatch):
    """tests/test_gpu_hf_parity.py for Qwen3: a safetensors checkpoint of a local
    ``Qwen3ForCausalLM`` loaded through ``EngineConfig(model_path=...)``."""
    transformers = pytest.importorskip("transformers")
    from dgi.engine import EngineConfig, LLMEngine
    from dgi.sched.request import SamplingParams
    cfg = transformers.Qwen3Config(vocab_size=V, hidden_size=H, intermediate_size=I, num_hidden_layers=L,
                                   num_attention_heads=NH, num_key_value_heads=NKV, head_dim=HD,
                                   max_position_embeddings=1024, rms_norm_eps=1e-6, bos_token_id=1, eos_token_id=2,
                                   tie_word_embeddings=False, rope_theta=1000000.0)
    model = transformers.Qwen3ForCausalLM(cfg)
    torch.manual_seed(0)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "norm" in n:
                p.copy_(1.0 + 0.1 * torch.randn_like(p))
            else:
                p.normal_(0.0, 0.04)
    model = model.eval().float()
    model.save_pretrained(str(tmp_path), safe_serialization=True)

    def engine(graphs):
        return LLMEngine(EngineConfig(model_path=str(tmp_path), device="cuda", dtype=torch.bfloat16, num_blocks=128,
                                      max_num_seqs=4, max_model_len=512, max_num_batched_tokens=256,
                                      use_graphs=graphs, enable_prefix_caching=False))
    calls = _count_op(monkeypatch)
    eng = engine(False)
    assert eng.model.cfg.qk_norm and eng.model.layers[0].q_norm.is_cuda
    sd = model.state_dict()
    assert torch.equal(eng.model.layers[1].k_norm.cpu(), sd["model.layers.1.self_attn.k_norm.weight"].bfloat16())
    steps = []
    orig = eng.model.compute_logits

    def spy(h, residual, idx):
        out = orig(h, residual, idx)
        steps.append(out.detach().float().cpu())
        return out

    eng.model.compute_logits = spy
    n_new = 12
    sp = SamplingParams(max_tokens=n_new, temperature=0.0, ignore_eos=True)
    worst = 0.0
    for prompt in HF_PROMPTS:
        steps.clear()
        toks = eng.generate([prompt], sp)[0].output
        assert len(toks) == n_new and len(steps) == n_new
        with torch.no_grad():
            ref = model(torch.tensor([prompt + toks])).logits[0]
        for t in range(n_new):
            r = ref[len(prompt) - 1 + t]
            g = steps[t][-1]
            tol = _tol(r)
            err = float((g - r).abs().max())
            worst = max(worst, err / tol)
            print(f"prompt {len(prompt)} step {t}: max |gpu - hf| {err:.4f}, tol {tol:.4f}")
            assert err <= tol, (len(prompt), t, err, tol)
            assert torch.nn.functional.cosine_similarity(g, r, dim=0) > 0.999, t
            assert float(r[toks[t]]) >= float(r.max()) - tol, (t, toks[t], int(r.argmax()))
    print(f"worst error / tol: {worst:.3f}")
    assert calls
    eng.model.compute_logits = orig
    geng = engine(True)
    eager = [r.output for r in eng.generate(HF_PROMPTS, sp)]
    graph = [r.output for r in geng.generate(HF_PROMPTS, sp)]
    assert graph == eager
