"""INT4 (group scale + zero point) weight-only quantisation on the GPU: the W4A16 skinny kernel, the
dequantiser, the routing of ``ops.linear`` and a quantised engine (the CPU side: test_int4_weights.py).
The oracle is the definition ``(code - zero) * scale``, written out here in fp64."""
import pytest
import torch

from dgi import ops
from dgi.ops import Int4Weight
from test_mxfp4_weights_gpu import _bf, _spy, _teacher_forced_ok

pytestmark = pytest.mark.gpu
DEV = "cuda"
# the skinny kernels' own (test_fp8_weights_gpu): exact weights, fp32 accumulation, one bf16 rounding
TOL = dict(atol=3e-2, rtol=2e-2)
MS = (1, 3, 16, 17, 32)
PROMPTS = [[1] + list(range(7, 7 + n - 1)) for n in (5, 40, 200, 7)]


@pytest.fixture(autouse=True, scope="module")
def _native():
    ops.load_native(required=True)


def _define(code, zero, scale):
    """(Int4Weight, its [N, K] definition in fp64) from plain codes [N, K], zeros and scales [N, K/128]."""
    w = (code - zero.repeat_interleave(128, 1)).double() * scale.double().repeat_interleave(128, 1)
    return Int4Weight.pack(code, zero, scale), w


_WEIGHTS = {}


def _weight(N, K):
    """Code byte (n, j) — elements 2j (low nibble) and 2j + 1 of the row — is (7n + j) % 256: every nibble
    pair, in every byte column.  zero (n + g) % 16 and scale 0.01 * 2^((n + 3g) % 8 - 4): one taken from the
    wrong row, group or lane is off by a factor of two at least.  Built once per shape, never changed."""
    if (N, K) not in _WEIGHTS:
        n = torch.arange(N, device=DEV)[:, None]
        byte = (7 * n + torch.arange(K // 2, device=DEV)[None, :]) % 256
        g = torch.arange(K // 128, device=DEV)[None, :]
        scale = (0.01 * torch.exp2(((n + 3 * g) % 8 - 4).float())).to(torch.float16)
        _WEIGHTS[N, K] = _define(torch.stack((byte & 15, byte >> 4), dim=-1).reshape(N, K), (n + g) % 16, scale)
    return _WEIGHTS[N, K]


def _ref(x, wd, bias=None):
    r = x.double() @ wd.t()
    return r if bias is None else r + bias.double()


@pytest.mark.parametrize("N,K", [(96, 1024), (256, 1024), (1152, 2048), (256, 14336)])
def test_skinny_gemm_i4(N, K):
    fw, wd = _weight(N, K)
    b = _bf(N)
    xs = {M: (_bf(M, K), _bf(M, K + 64)[:, :K]) for M in MS}
    refs = {(M, i, wb): _ref(x, wd, b if wb else None) for M in MS for i, x in enumerate(xs[M]) for wb in (0, 1)}
    ran, worst = 0, 0.0
    for cfg in [0] + sorted(ops.SKINNY_I4_CFGS):
        if not ops.skinny_i4_cfg_ok(cfg, N, K):
            # the kernel refuses a geometry that does not divide the shape instead of running part of it
            for M in (1, 32):
                out = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
                with pytest.raises(RuntimeError, match="code -5"):
                    torch.ops.dgi.skinny_gemm_i4(out, _bf(M, K), fw.q, fw.sz, None, cfg)
                assert not out.any()
            continue
        for M in MS:
            for i, x in enumerate(xs[M]):
                for wb in (0, 1):
                    out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
                    torch.ops.dgi.skinny_gemm_i4(out, x, fw.q, fw.sz, b if wb else None, cfg)
                    ref = refs[M, i, wb]
                    worst = max(worst, float(((out.double() - ref).abs() / (3e-2 + 2e-2 * ref.abs())).max()))
                    torch.testing.assert_close(out.double(), ref, **TOL,
                                               msg=lambda m: f"cfg {cfg} M {M} strided {i} bias {wb}: {m}")
                    ran += 1
    print(f"skinny_gemm_i4 {N}x{K}: worst error / tolerance {worst:.3f} over {ran} runs")
    assert ran >= 3 * len(MS) * 4       # the 4-wave one-tile configs (and the default) take every shape here


@pytest.mark.parametrize("M", [1, 17])
def test_skinny_gemm_i4_exact_k_order(M):
    """X of small integers (-2..2, four nonzero per group) against integer weights: every product and sum
    is an integer below 256, exact in fp32 and bf16, so any element paired with the wrong k shows."""
    N, K = 64, 2048
    gen = torch.Generator().manual_seed(3)
    n = torch.arange(N)[:, None]
    g = torch.arange(K // 128)[None, :]
    zero = (5 * n + g) % 16
    # codes within 3 of the zero point and scales 1 or 2 keep the 64 nonzero products of a row below 256
    code = (zero.repeat_interleave(128, 1) + torch.randint(-3, 4, (N, K), generator=gen)).clamp(0, 15)
    fw, wd = _define(code.to(DEV), zero.to(DEV), torch.exp2(((n + g) % 2).float()).to(torch.float16).to(DEV))
    x = torch.zeros(M, K // 128, 128)
    pos = torch.rand(M, K // 128, 128, generator=gen).argsort(dim=-1)[..., :4]
    sign = 2 * torch.randint(0, 2, pos.shape, generator=gen) - 1
    x.scatter_(2, pos, (torch.randint(1, 3, pos.shape, generator=gen) * sign).float())
    x = x.view(M, K).to(torch.bfloat16).to(DEV)
    ref = _ref(x, wd)
    assert 0 < float(ref.abs().max()) < 256 and torch.equal(ref, ref.round())
    for cfg in [0] + [c for c in sorted(ops.SKINNY_I4_CFGS) if ops.skinny_i4_cfg_ok(c, N, K)]:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
        torch.ops.dgi.skinny_gemm_i4(out, x, fw.q, fw.sz, None, cfg)
        assert torch.equal(out.double(), ref), cfg


@pytest.mark.parametrize("N,K", [(256, 1024), (48, 384)])
def test_dequant_int4_exact(N, K):
    """Bit-equal to the fp32 product rounded once (a 5-bit integer times an fp16 is exact in fp32)."""
    fw, wd = _weight(N, K)
    want = wd.float().to(torch.bfloat16)
    assert torch.equal(wd.float().double(), wd)
    out = torch.full((N, K), float("nan"), dtype=torch.bfloat16, device=DEV)
    torch.ops.dgi.dequant_int4(out, fw.q, fw.sz)
    assert torch.equal(out, want)
    scratch = torch.full((N * K + 4096,), float("nan"), dtype=torch.bfloat16, device=DEV)
    got = ops.dequant_int4(fw, scratch)
    assert got.data_ptr() == scratch.data_ptr() and torch.equal(got, want)
    assert torch.isnan(scratch[N * K:]).all()               # nothing written past the weight
    assert torch.equal(fw.dequant(torch.bfloat16), want)    # the torch decode on the GPU


def test_linear_routing(monkeypatch):
    """M <= 32 at K % 1024 == 0 runs the kernel; more rows, and an activation it cannot read, dequantise.
    Both against the exact weights.  The dequantised copy is rounded to bf16 (2^-9 relative per weight,
    2^-9 / sqrt(3) rms), which adds an error of 1.1e-3 of the output rms, 5e-3 of it at 4.5 sigma over these
    outputs: randn * 0.02 weights (output rms 0.9) keep that and the bf16 store (at most 2^-8 of an output
    below 4) well inside the tolerance.  On the kernel test's weights (output rms 15) the same rounding
    alone reaches 0.07, measured: the route is then outside this tolerance by design, not by fault."""
    names = _spy(monkeypatch)
    fw = ops.quantize_int4(_bf(1152, 2048, scale=0.02))
    wd = ((fw.codes().double() - fw.zeros().double().repeat_interleave(128, 1))
          * fw.scales().double().repeat_interleave(128, 1))
    b = _bf(1152)
    for M, op in ((8, "skinny_gemm_i4"), (32, "skinny_gemm_i4"), (33, "dequant_int4"), (300, "dequant_int4")):
        del names[:]
        x = _bf(M, 2048)
        torch.testing.assert_close(ops.linear(x, fw, b).double(), _ref(x, wd, b), **TOL)
        assert names == [op], (M, names)
    del names[:]
    x = _bf(4, 2048 + 4)[:, :2048]                          # rows not 16-byte aligned
    out = torch.empty(4, 1152, dtype=torch.bfloat16, device=DEV)
    assert ops.linear(x, fw, None, out) is out
    torch.testing.assert_close(out.double(), _ref(x, wd), **TOL)
    assert names == ["dequant_int4"]


def test_int4_engine_teacher_forced(monkeypatch):
    """llama-tiny-hd128 (H = 1024, I = 2048: decode rows take the int4 kernel) with int4 weights, eager and
    graph-replayed: all 40 tokens against an fp32 CPU model holding ``Int4Weight.dequant()``."""
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
                                     max_num_batched_tokens=256, use_graphs=graphs, weight_quant="awq"),
                        model_cfg=mc, model=gm)
        assert gm.weight_quant == "int4" and gm.act_quant is None and not gm.norms_folded
        assert all(isinstance(getattr(L, k), Int4Weight) and getattr(L, k).scratch is gm._quant_scratch
                   for L in gm.layers for k in QUANT_SLOTS)
        del names[:]
        outs[graphs] = [r.output for r in eng.generate(PROMPTS, sp)]
        assert "skinny_gemm_i4" in names and "dequant_int4" in names      # decode rows | prefill chunks
        assert not [n for n in names if n.startswith("mfma_gemm") or n in ("fused_skinny", "skinny_gemm_w8",
                                                                           "skinny_gemm_w4")]
        models[graphs] = gm
    f32 = LlamaModel(mc, "cpu", torch.float32, init="empty").copy_from(src)
    for L, Lq in zip(f32.layers, models[False].layers):
        for k in QUANT_SLOTS:
            getattr(L, k).copy_(getattr(Lq, k).dequant(torch.float32).cpu())
    assert _teacher_forced_ok(name, f32, PROMPTS, outs[False]) == 40
    assert outs[True] == outs[False]        # fixed reduction order: the graph replay computes the same tokens
