"""FP8 weight-only quantisation on the GPU: the W8A16 skinny kernel, the dequantiser, the routing
of ``ops.linear`` and a quantised engine (the CPU side: test_fp8_weights.py)."""
import pytest
import torch

from dgi import ops
from dgi.ops import Fp8Weight, quantize_fp8

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = dict(atol=3e-2, rtol=2e-2)       # test_skinny_gemm's: the widening is exact, the scale applied in fp32
MS = (1, 3, 16, 17, 32)
PROMPTS = [[1] + list(range(7, 7 + n - 1)) for n in (5, 40, 200, 7)]


@pytest.fixture(autouse=True, scope="module")
def _native():
    ops.load_native(required=True)


def _bf(*shape, scale=1.0):
    return (torch.randn(*shape, device=DEV) * scale).to(torch.bfloat16)


def _weight(N, K):
    """bf16 randn * 0.05, row n scaled by 2^((n % 8) - 4): a scale read from the wrong row or
    lane is off by a factor of two at least."""
    w = _bf(N, K, scale=0.05).float()
    w *= torch.exp2((torch.arange(N, device=DEV) % 8 - 4).float())[:, None]
    return quantize_fp8(w.to(torch.bfloat16))


def _every_code(N=256, K=1024):
    """Entry (n, k) holds byte (7n + k) % 256, the two NaN codes mapped to 0; scale 1."""
    n = torch.arange(N, device=DEV)[:, None]
    k = torch.arange(K, device=DEV)[None, :]
    b = ((7 * n + k) % 256).to(torch.uint8)
    b[(b == 0x7F) | (b == 0xFF)] = 0
    q = b.contiguous().view(torch.float8_e4m3fn)
    assert set(b.unique().tolist()) == set(range(256)) - {0x7F, 0xFF}
    return Fp8Weight(q, torch.ones(N, device=DEV))


def _ref(x, fw, bias=None):
    r = x.float() @ (fw.q.float() * fw.scale[:, None]).t()
    return r if bias is None else r + bias.float()


def _spy(monkeypatch):
    names = []
    orig = ops._call

    def call(name, *args):
        names.append(name)
        return orig(name, *args)
    monkeypatch.setattr(ops, "_call", call)
    return names


@pytest.mark.parametrize("N,K", [(96, 1024), (256, 1024), (1152, 2048), (512, 4096), (256, 14336)])
def test_skinny_gemm_w8(N, K):
    fw = _weight(N, K)
    b = _bf(N)
    ran = 0
    for cfg in [0] + sorted(ops.SKINNY_W8_CFGS):
        if not ops.skinny_w8_cfg_ok(cfg, N, K):
            # documented: column tiles per wave divide N / 16, waves x steps divide K / 128 — and the
            # kernel refuses the launch instead of running part of it
            out = torch.zeros(1, N, dtype=torch.bfloat16, device=DEV)
            with pytest.raises(RuntimeError, match="code -5"):
                torch.ops.dgi.skinny_gemm_w8(out, _bf(1, K), fw.q, fw.scale, None, cfg)
            assert not out.any()
            continue
        for M in MS:
            for x in (_bf(M, K), _bf(M, K + 64)[:, :K]):
                for bias in (None, b):
                    out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
                    torch.ops.dgi.skinny_gemm_w8(out, x, fw.q, fw.scale, bias, cfg)
                    torch.testing.assert_close(out.float(), _ref(x, fw, bias), **TOL,
                                               msg=lambda m: f"cfg {cfg} M {M} bias {bias is not None}: {m}")
                    ran += 1
    assert ran >= 5 * len(MS) * 4            # every shape here fits at least five of the configs


def test_skinny_gemm_w8_rejects_bad_operands():
    fw = _weight(96, 1024)
    out = torch.empty(1, 96, dtype=torch.bfloat16, device=DEV)
    x = _bf(1, 1024)
    with pytest.raises(RuntimeError, match="code -4"):
        torch.ops.dgi.skinny_gemm_w8(out, x, fw.q, fw.scale, None, 99)
    with pytest.raises(RuntimeError):
        torch.ops.dgi.skinny_gemm_w8(out, x, fw.q.view(torch.uint8), fw.scale, None, 0)
    with pytest.raises(RuntimeError):
        torch.ops.dgi.skinny_gemm_w8(out, x, fw.q, fw.scale[:95], None, 0)
    with pytest.raises(RuntimeError):
        torch.ops.dgi.skinny_gemm_w8(torch.empty(33, 96, dtype=torch.bfloat16, device=DEV), _bf(33, 1024), fw.q,
                                     fw.scale, None, 0)


@pytest.mark.parametrize("M", [1, 32])
def test_skinny_gemm_w8_every_code(M):
    """All 254 finite e4m3 codes in every lane position: an fnuz decode, dropped subnormals or a
    mishandled sign miss by far more than the tolerance."""
    fw = _every_code()
    x = _bf(M, 1024)
    for cfg in [0] + [c for c in sorted(ops.SKINNY_W8_CFGS) if ops.skinny_w8_cfg_ok(c, 256, 1024)]:
        out = torch.empty(M, 256, dtype=torch.bfloat16, device=DEV)
        torch.ops.dgi.skinny_gemm_w8(out, x, fw.q, fw.scale, None, cfg)
        torch.testing.assert_close(out.float(), _ref(x, fw), **TOL)


@pytest.mark.parametrize("case", ["48x1024", "1152x3584", "every_code"])
def test_dequant_fp8_exact(case):
    fw = _every_code() if case == "every_code" else _weight(*map(int, case.split("x")))
    N, K = fw.shape
    want = (fw.q.float() * fw.scale[:, None]).to(torch.bfloat16)
    out = torch.full((N, K), float("nan"), dtype=torch.bfloat16, device=DEV)
    torch.ops.dgi.dequant_fp8(out, fw.q, fw.scale)
    assert torch.equal(out, want)
    # through ops: into a larger flat scratch, and allocating one
    scratch = torch.full((N * K + 4096,), float("nan"), dtype=torch.bfloat16, device=DEV)
    got = ops.dequant_fp8(fw, scratch)
    assert got.data_ptr() == scratch.data_ptr() and torch.equal(got, want)
    assert torch.isnan(scratch[N * K:]).all()               # nothing written past the weight
    assert torch.equal(ops.dequant_fp8(fw), want)


def test_linear_routing(monkeypatch):
    """M > 32 and K = 3584 dequantise to bf16 and run the bf16 GEMM; M <= 32 at K % 1024 == 0 the kernel.

    Weights as in test_skinny_gemm (bf16 randn * 0.05, no per-row factor), which its tolerance is sized
    for: the dequant route rounds each dequantised weight to bf16 once more (2^-9 relative, by design),
    an error that grows with the row's magnitude — 8x rows would put ~0.02 rms on outputs of rms 18 and
    leave atol = 3e-2 to chance.  Rows and scales in the right place: test_dequant_fp8_exact."""
    names = _spy(monkeypatch)
    fw = quantize_fp8(_bf(1152, 2048, scale=0.05))
    b = _bf(1152)
    for M in (33, 300):
        x = _bf(M, 2048)
        torch.testing.assert_close(ops.linear(x, fw, b).float(), _ref(x, fw, b), **TOL)
    fw35 = quantize_fp8(_bf(1152, 3584, scale=0.05))
    x = _bf(1, 3584)
    out = torch.empty(1, 1152, dtype=torch.bfloat16, device=DEV)
    assert ops.linear(x, fw35, None, out) is out
    torch.testing.assert_close(out.float(), _ref(x, fw35), **TOL)
    assert "skinny_gemm_w8" not in names and names.count("dequant_fp8") == 3
    # a preallocated scratch is used as it is
    fw.scratch = torch.empty(1152 * 3584, dtype=torch.bfloat16, device=DEV)
    x = _bf(40, 2048)
    torch.testing.assert_close(ops.linear(x, fw).float(), _ref(x, fw), **TOL)
    del names[:]
    x = _bf(8, 2048)
    torch.testing.assert_close(ops.linear(x, fw, b).float(), _ref(x, fw, b), **TOL)
    assert names == ["skinny_gemm_w8"]
    # no K <= 4096 rule: the long-K down projection takes the kernel too
    del names[:]
    fwl = _weight(256, 14336)
    x = _bf(32, 14336)
    torch.testing.assert_close(ops.linear(x, fwl).float(), _ref(x, fwl), **TOL)
    assert names == ["skinny_gemm_w8"]


def _teacher_forced_ok(name, f32_model, prompts, gpu_outs, rel=0.03, abs_=0.02):
    """Every token the GPU chose is an argmax of the fp32 CPU model's logits for the same prefix
    (teacher forced), up to a bf16 tolerance — per step, every prompt (as in test_kernels_gpu)."""
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
            tol = rel * float(r.abs().max()) + abs_
            assert float(r[tok]) >= float(r.max()) - tol, (name, len(p), t, tok, int(r.argmax()))
            checked += 1
    return checked


def test_fp8_engine_teacher_forced(monkeypatch):
    """llama-tiny-hd128 (H = 1024, I = 2048: decode rows take the fp8 kernel) with fp8 weights, eager
    and graph-replayed: all 40 tokens against an fp32 CPU model holding the dequantised weights."""
    from dgi.engine import EngineConfig, LLMEngine
    from dgi.models.config import get_config
    from dgi.models.llama import QUANT_SLOTS, LlamaModel
    from dgi.sched.request import SamplingParams
    name = "llama-tiny-hd128"
    mc = get_config(name)
    src = LlamaModel(mc, "cpu", seed=5)
    sp = SamplingParams(max_tokens=10, temperature=0.0, ignore_eos=True)
    names = _spy(monkeypatch)
    outs, models = {}, {}
    for graphs in (False, True):
        gm = LlamaModel(mc, "cuda", init="empty").copy_from(src)
        eng = LLMEngine(EngineConfig(model=name, device="cuda", num_blocks=256, max_num_seqs=8, max_model_len=512,
                                     max_num_batched_tokens=256, use_graphs=graphs, weight_quant="fp8"),
                        model_cfg=mc, model=gm)
        assert gm.weight_quant == "fp8" and eng.mlp_pad_table is None and not gm.norms_folded
        assert gm._quant_scratch.numel() == max(getattr(gm.layers[0], k).q.numel() for k in QUANT_SLOTS)
        del names[:]
        outs[graphs] = [r.output for r in eng.generate(PROMPTS, sp)]
        assert "skinny_gemm_w8" in names and "dequant_fp8" in names      # decode rows | prefill chunks
        # none of the layer kernels that read bf16 weights (skinny_gemm may serve the bf16 lm_head)
        assert not {"fused_skinny", "mfma_gemm", "mfma_gemm_norm", "mfma_gemm_norm_rope"} & set(names)
        models[graphs] = gm
    assert all(len(o) == 10 for o in outs[False])
    # the fp32 CPU model holding exactly the weights the GPU engine serves
    f32 = LlamaModel(mc, "cpu", torch.float32, init="empty").copy_from(src)
    for L, Lq in zip(f32.layers, models[False].layers):
        for k in QUANT_SLOTS:
            fw = getattr(Lq, k)
            getattr(L, k).copy_(Fp8Weight(fw.q.cpu(), fw.scale.cpu()).dequant(torch.float32))
    assert _teacher_forced_ok(name, f32, PROMPTS, outs[False]) == 40
    # fixed reduction order: the graph replay computes the same tokens
    assert outs[True] == outs[False]
