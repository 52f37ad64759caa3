"""Block-scaled FP8 on the GPU: the W8A16 kernel over [N/16, K/128] scales, its dequantiser, the routing of
``ops.linear`` and an engine over a block-FP8 checkpoint (the CPU side: test_fp8_block.py)."""
import json

import pytest
import torch

from dgi import ops
from dgi.ops import Fp8BlockWeight

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = dict(atol=3e-2, rtol=2e-2)       # test_fp8_weights_gpu's: exact products, fp32 accumulation, one bf16 rounding
SHAPES = [(96, 1024), (256, 1024), (1152, 2048), (256, 14336)]
E4M3 = torch.float8_e4m3fn


@pytest.fixture(autouse=True, scope="module")
def _native():
    ops.load_native(required=True)


def _bf(*shape, scale=1.0):
    return (torch.randn(*shape, device=DEV) * scale).to(torch.bfloat16)


def _cfgs(N, K):
    return [0] + [c for c in sorted(ops.SKINNY_W8_CFGS) if ops.skinny_w8_cfg_ok(c, N, K)]


def _expand(scale, N, K):
    return scale.repeat_interleave(16, 0).repeat_interleave(128, 1)


def _ref(x, fw, bias=None):
    """The definition in fp64, on the CPU: x (q * scale of the element's tile and step)^T + bias."""
    r = x.cpu().double() @ (fw.q.cpu().double() * _expand(fw.scale.cpu(), *fw.shape).double()).t()
    return r if bias is None else r + bias.cpu().double()


def _run(x, fw, bias, cfg):
    out = torch.full((x.shape[0], fw.shape[0]), float("nan"), dtype=torch.bfloat16, device=DEV)
    torch.ops.dgi.skinny_gemm_w8b(out, x, fw.q, fw.scale, bias, cfg)
    return out.cpu().double()


def _real_weight(N, K, pattern=False):
    """test_fp8_weights_gpu's weights (bf16 randn * 0.05, row n times 2^((n % 8) - 4)) cut into 16 x 128 blocks of
    scale max|block| / 448: real scales, none a power of two.  ``pattern``: its every-code bytes instead (entry
    (n, k) holds byte (7n + k) % 256, the two NaN codes mapped to 0) under scales 0.5 + 0.37 ((tile + 2 step) % 4)."""
    if pattern:
        b = ((7 * torch.arange(N, device=DEV)[:, None] + torch.arange(K, device=DEV)[None, :]) % 256).to(torch.uint8)
        b[(b == 0x7F) | (b == 0xFF)] = 0
        assert set(b.unique().tolist()) == set(range(256)) - {0x7F, 0xFF}
        t, s = torch.arange(N // 16, device=DEV)[:, None], torch.arange(K // 128, device=DEV)[None, :]
        return Fp8BlockWeight(b.contiguous().view(E4M3), (0.5 + 0.37 * ((t + 2 * s) % 4)).float().contiguous())
    w = _bf(N, K, scale=0.05).float() * torch.exp2((torch.arange(N, device=DEV) % 8 - 4).float())[:, None]
    blocks = w.view(N // 16, 16, K // 128, 128)
    scale = (blocks.abs().amax(dim=(1, 3)) / 448.0).contiguous()
    q = (blocks / scale[:, None, :, None]).clamp_(-448, 448).view(N, K).to(E4M3)
    return Fp8BlockWeight(q, scale)


@pytest.mark.parametrize("M", [1, 16, 17, 32])
@pytest.mark.parametrize("N,K", SHAPES)
def test_exact_answers(N, K, M):
    """Integers against power-of-two scales 2^((tile + 3 step) % 5 - 2): a scale from a neighbouring tile or step
    is off by a factor of two at least, and every output must equal the fp64 result bit for bit.  Codes are dense
    integers in [-3, 3]; row m of X holds 2, -1, 1, -1 in steps 4m .. 4m + 3 (mod K / 128, lane position
    37m + 11j) and zeros elsewhere; the bias is an integer in [-3, 3].  An output is then a multiple of 1/4 of
    magnitude at most 5 * 3 * 4 + 3 = 63 < 64, which bf16's 8 significant bits hold exactly (a multiple of 1/4
    below 256, as every partial sum is, is exact in fp32 but not always in bf16).  32 rows touch 128 consecutive
    steps, every step of every shape here."""
    g = torch.Generator().manual_seed(N + K)
    S = K // 128
    q = torch.randint(-3, 4, (N, K), generator=g).float()
    t, s = torch.arange(N // 16)[:, None], torch.arange(S)[None, :]
    fw = Fp8BlockWeight(q.to(E4M3).to(DEV), torch.exp2(((t + 3 * s) % 5 - 2).float()).contiguous().to(DEV))
    x = torch.zeros(M, K + 64)
    for m in range(M):
        for j, v in enumerate((2.0, -1.0, 1.0, -1.0)):
            x[m, 128 * ((4 * m + j) % S) + (37 * m + 11 * j) % 128] = v
    bias = torch.randint(-3, 4, (N,), generator=g).to(torch.bfloat16).to(DEV)
    xs = x.to(torch.bfloat16).to(DEV)[:, :K]                  # rows 64 elements apart from contiguous
    for xv, b in ((xs.contiguous(), None), (xs, bias)):
        want = _ref(xv, fw, b)
        assert (want * 4 == (want * 4).round()).all() and float(want.abs().max()) < 256
        assert torch.equal(want.to(torch.bfloat16).double(), want) and want.any()
        for cfg in _cfgs(N, K):
            assert torch.equal(_run(xv, fw, b, cfg), want), (cfg, b is not None)


@pytest.mark.parametrize("N,K", SHAPES)
def test_random_values(N, K):
    fw, b = _real_weight(N, K), _bf(N)
    for M in (1, 3, 16, 17, 32):
        x = _bf(M, K)
        for cfg in _cfgs(N, K):
            for bias in (None, b):
                torch.testing.assert_close(_run(x, fw, bias, cfg), _ref(x, fw, bias), **TOL,
                                           msg=lambda m: f"cfg {cfg} M {M} bias {bias is not None}: {m}")


@pytest.mark.parametrize("M", [1, 32])
def test_every_code(M):
    """All 254 finite e4m3 codes in every lane position: an fnuz decode, dropped subnormals or a mishandled sign
    miss by far more than the tolerance."""
    fw, x = _real_weight(256, 1024, pattern=True), _bf(M, 1024)
    for cfg in _cfgs(256, 1024):
        torch.testing.assert_close(_run(x, fw, None, cfg), _ref(x, fw), **TOL)


@pytest.mark.parametrize("case", ["48x1024", "1152x3584", "every_code"])
def test_dequant_fp8_block_exact(case):
    fw = _real_weight(256, 1024, pattern=True) if case == "every_code" else _real_weight(*map(int, case.split("x")))
    N, K = fw.shape
    want = (fw.q.float() * _expand(fw.scale, N, K)).to(torch.bfloat16)
    scratch = torch.full((N * K + 4096,), float("nan"), dtype=torch.bfloat16, device=DEV)
    got = ops.dequant_fp8_block(fw, scratch)
    assert got.data_ptr() == scratch.data_ptr() and torch.equal(got, want)
    assert torch.isnan(scratch[N * K:]).all()               # nothing written past the weight
    assert torch.equal(ops.dequant_fp8_block(fw), want)


def test_linear_routing(monkeypatch):
    """Decode-sized steps at K % 1024 == 0 take the kernel; M > 32 and K = 3584 dequantise and run the bf16 GEMM.
    Weights without the per-row factor, as in test_fp8_weights_gpu's routing test: the dequantised route rounds
    each weight to bf16 once more, which the tolerance is not sized for on 8x rows."""
    names = []
    orig = ops._call
    monkeypatch.setattr(ops, "_call", lambda name, *a: (names.append(name), orig(name, *a))[1])

    def weight(N, K):
        q, s = ops.quantize_fp8_block_hf(_bf(N, K, scale=0.05))
        return ops.fp8_block_from_hf(q, s)
    fw, fw35, b = weight(1152, 2048), weight(1152, 3584), _bf(1152)
    for M, w, op in ((8, fw, "skinny_gemm_w8b"), (32, fw, "skinny_gemm_w8b"), (33, fw, "dequant_fp8_block"),
                     (300, fw, "dequant_fp8_block"), (1, fw35, "dequant_fp8_block")):
        del names[:]
        x = _bf(M, w.shape[1])
        torch.testing.assert_close(ops.linear(x, w, b).cpu().double(), _ref(x, w, b), **TOL)
        assert names == [op], (M, names)


def test_rejects_bad_operands():
    fw = _real_weight(96, 1024)
    x = _bf(1, 1024)
    out = torch.zeros(1, 96, dtype=torch.bfloat16, device=DEV)
    big = torch.zeros(33, 96, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="code -4"):
        torch.ops.dgi.skinny_gemm_w8b(out, x, fw.q, fw.scale, None, 99)
    for o, xx, q, s in ((out, x, fw.q.view(torch.uint8), fw.scale), (out, x, fw.q, fw.scale[:5]),
                        (out, x, fw.q, fw.scale.double()), (big, _bf(33, 1024), fw.q, fw.scale)):
        with pytest.raises(RuntimeError):
            torch.ops.dgi.skinny_gemm_w8b(o, xx, q, s, None, 0)
    with pytest.raises(RuntimeError):
        torch.ops.dgi.dequant_fp8_block(torch.zeros(96, 1024, dtype=torch.bfloat16, device=DEV), fw.q, fw.scale[:5])
    assert not out.any() and not big.any()


def _teacher_forced_ok(name, f32_model, prompts, gpu_outs, rel=0.03, abs_=0.02):
    """test_fp8_weights_gpu's check and bound: every token the GPU chose is an argmax of the fp32 CPU model's
    logits for the same prefix, up to a bf16 tolerance."""
    from dgi.engine import EngineConfig, LLMEngine
    from dgi.sched.request import SamplingParams
    ref = LLMEngine(EngineConfig(model=name, device="cpu", dtype=torch.float32, num_blocks=256, max_num_seqs=8,
                                 max_model_len=512, max_num_batched_tokens=256, use_graphs=False,
                                 enable_prefix_caching=False), model_cfg=f32_model.cfg, model=f32_model)
    got = {}
    orig = ref.model.compute_logits

    def spy(h, residual, idx):
        out = orig(h, residual, idx)
        got["l"] = out[-1].detach().float()
        return out
    ref.model.compute_logits = spy
    one = SamplingParams(max_tokens=1, temperature=0.0, ignore_eos=True)
    checked = 0
    for p, toks in zip(prompts, gpu_outs):
        for t, tok in enumerate(toks):
            ref.generate([p + toks[:t]], one)
            r = got["l"]
            assert float(r[tok]) >= float(r.max()) - (rel * float(r.abs().max()) + abs_), (len(p), t, tok, int(r.argmax()))
            checked += 1
    return checked


def test_engine_from_checkpoint(tmp_path):
    """llama-tiny-hd128 written as a block-FP8 checkpoint (128 x 128 scales, bf16 LM head), loaded on the GPU,
    eager and graph-replayed: 2 prompts x 20 tokens against an fp32 CPU model holding the decoded weights."""
    from safetensors.torch import save_file
    from dgi.engine import EngineConfig, LLMEngine
    from dgi.models.config import get_config
    from dgi.models.llama import QUANT_SLOTS, LlamaModel
    from dgi.sched.request import SamplingParams
    name = "llama-tiny-hd128"
    mc = get_config(name)
    src = LlamaModel(mc, "cpu", seed=5)
    ql, kl, I = mc.num_heads * mc.head_dim, mc.num_kv_heads * mc.head_dim, mc.intermediate_size
    sd = {"model.embed_tokens.weight": src.embed, "model.norm.weight": src.norm, "lm_head.weight": src.lm_head.clone()}
    for li, L in enumerate(src.layers):
        p = f"model.layers.{li}."
        sd[p + "input_layernorm.weight"], sd[p + "post_attention_layernorm.weight"] = L.in_norm, L.post_norm
        for k, w in (("self_attn.q_proj", L.qkv[:ql]), ("self_attn.k_proj", L.qkv[ql:ql + kl]),
                     ("self_attn.v_proj", L.qkv[ql + kl:]), ("self_attn.o_proj", L.o), ("mlp.gate_proj", L.gate_up[:I]),
                     ("mlp.up_proj", L.gate_up[I:]), ("mlp.down_proj", L.down)):
            sd[p + k + ".weight"], sd[p + k + ".weight_scale_inv"] = ops.quantize_fp8_block_hf(w)
    try:
        save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / "model.safetensors"))
    except Exception as e:      # pragma: no cover - depends on the installed safetensors
        pytest.skip(f"the installed safetensors cannot write float8_e4m3fn: {e!r}")
    (tmp_path / "config.json").write_text(json.dumps({"quantization_config": {
        "quant_method": "fp8", "fmt": "e4m3", "weight_block_size": [128, 128], "activation_scheme": "dynamic",
        "modules_to_not_convert": ["lm_head"]}}))
    prompts = [[1] + list(range(7, 11)), [1] + list(range(7, 46))]
    sp = SamplingParams(max_tokens=20, temperature=0.0, ignore_eos=True)
    outs = {}
    for graphs in (False, True):
        eng = LLMEngine(EngineConfig(model=name, model_path=str(tmp_path), device="cuda", num_blocks=256, max_num_seqs=8,
                                     max_model_len=512, max_num_batched_tokens=256, use_graphs=graphs,
                                     weight_quant="fp8"), model_cfg=mc)
        gm = eng.model
        assert gm.weight_quant == "fp8" and all(isinstance(getattr(L, k), Fp8BlockWeight)
                                                for L in gm.layers for k in QUANT_SLOTS)
        outs[graphs] = [r.output for r in eng.generate(prompts, sp)]
    f32 = LlamaModel(mc, "cpu", torch.float32, init="empty").copy_from(src)
    for L, Lq in zip(f32.layers, gm.layers):
        for k in QUANT_SLOTS:
            fw = getattr(Lq, k)
            getattr(L, k).copy_(Fp8BlockWeight(fw.q.cpu(), fw.scale.cpu()).dequant(torch.float32))
    assert _teacher_forced_ok(name, f32, prompts, outs[False]) == 40
    assert outs[True] == outs[False]        # fixed reduction order: the graph replay computes the same tokens
