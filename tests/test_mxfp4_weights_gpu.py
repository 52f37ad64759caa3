"""MXFP4 weight-only quantisation on the GPU: the W4A16 skinny kernel, the dequantiser, the routing
of ``ops.linear`` and a quantised engine (the CPU side: test_mxfp4_weights.py).  The oracle is the
OCP e2m1 table, written out here."""
import pytest
import torch

from dgi import ops
from dgi.ops import Mxfp4Weight, quantize_mxfp4

pytestmark = pytest.mark.gpu
DEV = "cuda"
# test_fp8_weights_gpu's (test_skinny_gemm's): the same error sources — an exact widening, fp32
# accumulation, one bf16 rounding — on outputs of comparable magnitude (rms ~20 at K = 14336)
TOL = dict(atol=3e-2, rtol=2e-2)
MS = (1, 3, 16, 17, 32)
PROMPTS = [[1] + list(range(7, 7 + n - 1)) for n in (5, 40, 200, 7)]
GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)      # e2m1 magnitudes by code 0..7; bit 3 is the sign


@pytest.fixture(autouse=True, scope="module")
def _native():
    ops.load_native(required=True)


def _bf(*shape, scale=1.0):
    return (torch.randn(*shape, device=DEV) * scale).to(torch.bfloat16)


def _decode(fw):
    """The weight in fp32 from the table above (exact): low nibble first, 2^(scale - 127) per 32 elements."""
    table = torch.tensor(GRID + tuple(-v for v in GRID), dtype=torch.float32, device=fw.q.device)
    N, K = fw.q.shape[0], 2 * fw.q.shape[1]
    codes = torch.stack((fw.q & 15, fw.q >> 4), dim=-1).reshape(N, K).long()
    s = torch.exp2(fw.scale.float() - 127).repeat_interleave(32, dim=1)
    return table[codes] * s


_WEIGHTS = {}


def _weight(N, K):
    """bf16 randn * 0.05, block (n, kb) scaled by 2^((n + kb) % 8 - 4): a scale taken from the wrong
    row, block or lane is off by a factor of two at least.  Built once per shape, never changed."""
    if (N, K) not in _WEIGHTS:
        w = _bf(N, K, scale=0.05).float().view(N, K // 32, 32)
        n = torch.arange(N, device=DEV)[:, None]
        kb = torch.arange(K // 32, device=DEV)[None, :]
        w = w * torch.exp2(((n + kb) % 8 - 4).float())[:, :, None]
        fw = quantize_mxfp4(w.view(N, K).to(torch.bfloat16))
        assert len(fw.scale.unique()) >= 8
        _WEIGHTS[N, K] = (fw, _decode(fw))
    return _WEIGHTS[N, K]


def _every_code(N=256, K=1024):
    """Byte (n, j) is (7n + j) % 256: all 256 nibble pairs, in every byte column; scale code 127."""
    if "every" not in _WEIGHTS:
        n = torch.arange(N, device=DEV)[:, None]
        j = torch.arange(K // 2, device=DEV)[None, :]
        q = ((7 * n + j) % 256).to(torch.uint8).contiguous()
        assert set(q.unique().tolist()) == set(range(256))
        assert all(len(q[:, c].unique()) == 256 for c in range(0, K // 2, 37))     # 7 is odd: every column
        fw = Mxfp4Weight(q, torch.full((N, K // 32), 127, dtype=torch.uint8, device=DEV))
        _WEIGHTS["every"] = (fw, _decode(fw))
    return _WEIGHTS["every"]


def _scale_sweep(N=64, K=1024):
    """Random codes under scale codes sweeping 2..252 (every code of the specified range)."""
    q = torch.randint(0, 256, (N, K // 2), device=DEV, dtype=torch.uint8)
    s = (2 + torch.arange(N * (K // 32), device=DEV) % 251).to(torch.uint8).view(N, K // 32)
    assert set(s.unique().tolist()) == set(range(2, 253))
    fw = Mxfp4Weight(q, s)
    return fw, _decode(fw)


def _ref(x, wf, bias=None):
    r = x.float() @ wf.t()
    return r if bias is None else r + bias.float()


def _spy(monkeypatch):
    names = []
    orig = ops._call

    def call(name, *args):
        names.append(name)
        return orig(name, *args)
    monkeypatch.setattr(ops, "_call", call)
    return names


@pytest.mark.parametrize("N,K", [(96, 1024), (256, 1024), (1152, 2048), (256, 14336)])
def test_skinny_gemm_w4(N, K):
    fw, wf = _weight(N, K)
    b = _bf(N)
    xs = {M: (_bf(M, K), _bf(M, K + 64)[:, :K]) for M in MS}
    refs = {(M, i, wb): _ref(x, wf, b if wb else None) for M in MS for i, x in enumerate(xs[M]) for wb in (0, 1)}
    ran = 0
    for cfg in [0] + sorted(ops.SKINNY_W4_CFGS):
        if not ops.skinny_w4_cfg_ok(cfg, N, K):
            # documented: column tiles per wave divide N / 16, waves x steps divide K / 256 — and the
            # kernel refuses the launch instead of running part of it
            for M in (1, 32):
                out = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
                with pytest.raises(RuntimeError, match="code -5"):
                    torch.ops.dgi.skinny_gemm_w4(out, _bf(M, K), fw.q, fw.scale, None, cfg)
                assert not out.any()
            continue
        for M in MS:
            for i, x in enumerate(xs[M]):
                for wb in (0, 1):
                    out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
                    torch.ops.dgi.skinny_gemm_w4(out, x, fw.q, fw.scale, b if wb else None, cfg)
                    torch.testing.assert_close(out.float(), refs[M, i, wb], **TOL,
                                               msg=lambda m: f"cfg {cfg} M {M} strided {i} bias {wb}: {m}")
                    ran += 1
    # the 4-wave one-tile configs (and the default) take every shape here
    assert ran >= 3 * len(MS) * 4


def test_skinny_gemm_w4_rejects_bad_operands():
    fw, _ = _weight(96, 1024)
    out = torch.empty(1, 96, dtype=torch.bfloat16, device=DEV)
    x = _bf(1, 1024)
    with pytest.raises(RuntimeError, match="code -4"):
        torch.ops.dgi.skinny_gemm_w4(out, x, fw.q, fw.scale, None, 99)
    with pytest.raises(RuntimeError):       # M = 33
        torch.ops.dgi.skinny_gemm_w4(torch.empty(33, 96, dtype=torch.bfloat16, device=DEV), _bf(33, 1024), fw.q,
                                     fw.scale, None, 0)
    with pytest.raises(RuntimeError):       # codes of another dtype
        torch.ops.dgi.skinny_gemm_w4(out, x, fw.q.view(torch.int8), fw.scale, None, 0)
    with pytest.raises(RuntimeError):
        torch.ops.dgi.skinny_gemm_w4(out, x, fw.q, fw.scale.float(), None, 0)
    with pytest.raises(RuntimeError):
        torch.ops.dgi.skinny_gemm_w4(out, x.float(), fw.q, fw.scale, None, 0)
    with pytest.raises(RuntimeError):       # a short scale: rows, then blocks
        torch.ops.dgi.skinny_gemm_w4(out, x, fw.q, fw.scale[:95], None, 0)
    with pytest.raises(RuntimeError):
        torch.ops.dgi.skinny_gemm_w4(out, x, fw.q, fw.scale[:, :31].contiguous(), None, 0)
    with pytest.raises(RuntimeError):       # K of x against K of the weight
        torch.ops.dgi.skinny_gemm_w4(out, _bf(1, 2048), fw.q, fw.scale, None, 0)
    full = torch.full((96, 1024), float("nan"), dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError):
        torch.ops.dgi.dequant_mxfp4(full, fw.q, fw.scale[:, :31].contiguous())
    with pytest.raises(RuntimeError):
        torch.ops.dgi.dequant_mxfp4(full.float(), fw.q, fw.scale)
    with pytest.raises(RuntimeError):
        torch.ops.dgi.dequant_mxfp4(full[:, :512].contiguous(), fw.q, fw.scale)
    assert torch.isnan(full).all()


@pytest.mark.parametrize("M", [1, 32])
def test_skinny_gemm_w4_every_code(M):
    """All 256 code pairs under the kernel: swapped nibbles, a wrong table entry or a dropped sign
    miss by far more than the tolerance (entries are up to 6, rows of 1024)."""
    fw, wf = _every_code()
    x = _bf(M, 1024)
    ref = _ref(x, wf)
    ran = 0
    for cfg in [0] + [c for c in sorted(ops.SKINNY_W4_CFGS) if ops.skinny_w4_cfg_ok(c, 256, 1024)]:
        out = torch.empty(M, 256, dtype=torch.bfloat16, device=DEV)
        torch.ops.dgi.skinny_gemm_w4(out, x, fw.q, fw.scale, None, cfg)
        torch.testing.assert_close(out.float(), ref, **TOL, msg=lambda m: f"cfg {cfg}: {m}")
        ran += 1
    assert ran >= 5


@pytest.mark.parametrize("case", ["48x1024", "1152x3584", "every_code", "scale_sweep"])
def test_dequant_mxfp4_exact(case):
    fw, wf = (_every_code() if case == "every_code" else _scale_sweep() if case == "scale_sweep"
              else _weight(*map(int, case.split("x"))))
    N, K = fw.shape
    want = wf.to(torch.bfloat16)
    assert torch.equal(want.float(), wf)                    # the format's values are bf16 numbers
    out = torch.full((N, K), float("nan"), dtype=torch.bfloat16, device=DEV)
    torch.ops.dgi.dequant_mxfp4(out, fw.q, fw.scale)
    assert torch.equal(out, want)
    # through ops: into a larger flat scratch, and allocating one
    scratch = torch.full((N * K + 4096,), float("nan"), dtype=torch.bfloat16, device=DEV)
    got = ops.dequant_mxfp4(fw, scratch)
    assert got.data_ptr() == scratch.data_ptr() and torch.equal(got, want)
    assert torch.isnan(scratch[N * K:]).all()               # nothing written past the weight
    assert torch.equal(ops.dequant_mxfp4(fw), want)
    assert torch.equal(fw.dequant(torch.bfloat16), want)    # the torch decode on the GPU


def test_linear_routing(monkeypatch):
    """M > 32 and K = 3584 dequantise to bf16 and run the bf16 GEMM; M <= 32 at K % 1024 == 0 the
    kernel.  The dequantised weight is exact, so both routes multiply the same numbers."""
    names = _spy(monkeypatch)
    fw, wf = _weight(1152, 2048)
    b = _bf(1152)
    for M in (33, 300):
        x = _bf(M, 2048)
        torch.testing.assert_close(ops.linear(x, fw, b).float(), _ref(x, wf, b), **TOL)
    fw35, wf35 = _weight(1152, 3584)
    x = _bf(1, 3584)
    out = torch.empty(1, 1152, dtype=torch.bfloat16, device=DEV)
    assert ops.linear(x, fw35, None, out) is out
    torch.testing.assert_close(out.float(), _ref(x, wf35), **TOL)
    assert "skinny_gemm_w4" not in names and names.count("dequant_mxfp4") == 3
    # a preallocated scratch is used as it is
    big = Mxfp4Weight(fw.q, fw.scale, torch.full((1152 * 3584,), float("nan"), dtype=torch.bfloat16, device=DEV))
    x = _bf(40, 2048)
    torch.testing.assert_close(ops.linear(x, big).float(), _ref(x, wf), **TOL)
    assert torch.equal(big.scratch[:1152 * 2048].view(1152, 2048).float(), wf)      # the exact weight, in place
    assert torch.isnan(big.scratch[1152 * 2048:]).all()
    del names[:]
    x = _bf(8, 2048)
    torch.testing.assert_close(ops.linear(x, fw, b).float(), _ref(x, wf, b), **TOL)
    assert names == ["skinny_gemm_w4"]
    # no K <= 4096 rule: the long-K down projection takes the kernel too
    del names[:]
    fwl, wfl = _weight(256, 14336)
    x = _bf(32, 14336)
    got = ops.linear(x, fwl)
    torch.testing.assert_close(got.float(), _ref(x, wfl), **TOL)
    assert names == ["skinny_gemm_w4"]
    # both routes on the same (x, w)
    other = torch.nn.functional.linear(x, ops.dequant_mxfp4(fwl))
    torch.testing.assert_close(got.float(), other.float(), **TOL)
    # an activation the kernel cannot read (rows not 16-byte aligned) takes the dequant route
    del names[:]
    x = _bf(4, 2048 + 4)[:, :2048]
    torch.testing.assert_close(ops.linear(x, fw).float(), _ref(x, wf), **TOL)
    assert names == ["dequant_mxfp4"]


def _teacher_forced_ok(name, f32_model, prompts, gpu_outs, rel=0.03, abs_=0.02, kv_dtype=None):
    """Every token the GPU chose is an argmax of the fp32 CPU model's logits for the same prefix
    (teacher forced), up to a bf16 tolerance — per step, every prompt (as in test_fp8_weights_gpu; with
    ``kv_dtype`` the reference engine runs on the same kind of KV pool, as in test_kv_fp8_gpu)."""
    from dgi.engine import EngineConfig, LLMEngine
    from dgi.sched.request import SamplingParams
    ref = LLMEngine(EngineConfig(model=name, device="cpu", dtype=torch.float32, num_blocks=256, max_num_seqs=8,
                                 max_model_len=512, max_num_batched_tokens=256, use_graphs=False,
                                 enable_prefix_caching=False, kv_dtype=kv_dtype), model_cfg=f32_model.cfg,
                    model=f32_model)
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


@pytest.mark.parametrize("kv_dtype", [None, "fp8"])
def test_mxfp4_engine_teacher_forced(kv_dtype, monkeypatch):
    """llama-tiny-hd128 (H = 1024, I = 2048: decode rows take the mxfp4 kernel) with mxfp4 weights,
    eager and graph-replayed: all 40 tokens against an fp32 CPU model holding the dequantised weights.
    ``kv_dtype="fp8"``: the same on an e4m3 KV pool (a single-GPU engine composes the two)."""
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
                                     max_num_batched_tokens=256, use_graphs=graphs, weight_quant="mxfp4",
                                     kv_dtype=kv_dtype), model_cfg=mc, model=gm)
        assert gm.kv_fp8 == (kv_dtype == "fp8") and (eng.pool.dtype == torch.float8_e4m3fn) == (kv_dtype == "fp8")
        assert gm.weight_quant == "mxfp4" and gm.act_quant is None and eng.mlp_pad_table is None
        assert not gm.norms_folded
        largest = max(getattr(gm.layers[0], k).shape[0] * getattr(gm.layers[0], k).shape[1] for k in QUANT_SLOTS)
        assert gm._quant_scratch.numel() == largest and gm._quant_scratch.dtype == torch.bfloat16
        assert all(isinstance(getattr(L, k), Mxfp4Weight) and getattr(L, k).scratch is gm._quant_scratch
                   for L in gm.layers for k in QUANT_SLOTS)
        del names[:]
        outs[graphs] = [r.output for r in eng.generate(PROMPTS, sp)]
        assert "skinny_gemm_w4" in names and "dequant_mxfp4" in names      # decode rows | prefill chunks
        # none of the layer kernels that read bf16 or fp8 weights (skinny_gemm may serve the bf16 lm_head)
        assert not [n for n in names if n.startswith("mfma_gemm") or n in ("fused_skinny", "skinny_gemm_w8",
                                                                           "dequant_fp8")]
        models[graphs] = gm
    assert all(len(o) == 10 for o in outs[False])
    # the fp32 CPU model holding exactly the weights the GPU engine serves
    f32 = LlamaModel(mc, "cpu", torch.float32, init="empty").copy_from(src)
    for L, Lq in zip(f32.layers, models[False].layers):
        for k in QUANT_SLOTS:
            fw = getattr(Lq, k)
            getattr(L, k).copy_(_decode(Mxfp4Weight(fw.q.cpu(), fw.scale.cpu())))
    assert _teacher_forced_ok(name, f32, PROMPTS, outs[False], kv_dtype=kv_dtype) == 40
    # fixed reduction order: the graph replay computes the same tokens
    assert outs[True] == outs[False]
