"""FP8 W8A8 projections on the GPU: the row quantiser (bit-exact), the e4m3 MFMA GEMM (exact
integers, every finite code, random data), the routing of ``ops.linear`` and a W8A8 engine
(the CPU side: test_w8a8.py)."""
import pytest
import torch

from dgi import ops
from dgi.ops import Fp8Weight, quantize_fp8

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = dict(atol=3e-2, rtol=2e-2)       # test_fp8_weights_gpu's, for the act=None routes
PROMPTS = [[1] + list(range(7, 7 + n - 1)) for n in (5, 40, 200, 7)]
F8 = torch.float8_e4m3fn


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


def _codes(N, K, a, b):
    """Entry (n, k) holds byte (a n + b k) % 256, the two NaN codes mapped to 0."""
    n = torch.arange(N, device=DEV)[:, None]
    k = torch.arange(K, device=DEV)[None, :]
    c = ((a * n + b * k) % 256).to(torch.uint8)
    c[(c == 0x7F) | (c == 0xFF)] = 0
    assert set(c.unique().tolist()) == set(range(256)) - {0x7F, 0xFF}
    return c.contiguous().view(F8)


def _every_code(N=256, K=1024):
    return Fp8Weight(_codes(N, K, 7, 1), torch.ones(N, device=DEV))


def _spy(monkeypatch):
    names = []
    orig = ops._call

    def call(name, *args):
        names.append(name)
        return orig(name, *args)
    monkeypatch.setattr(ops, "_call", call)
    return names


def _gemm(xq, sx, wq, sw, bias=None):
    out = torch.full((xq.shape[0], wq.shape[0]), float("nan"), dtype=torch.bfloat16, device=DEV)
    torch.ops.dgi.mfma_gemm_fp8(out, xq, sx, wq, sw, bias)
    return out


# ---------------------------------------------------------------------------- quantiser

@pytest.mark.parametrize("K", [16, 128, 1024, 2048, 2064, 3584])     # one wave per row up to 2048, four above
def test_quant_rows_fp8_exact(K):
    """Codes and scales bit for bit, contiguous and strided rows; rows scaled by 2^((m % 8) - 4) so a
    scale taken from another row is off by 2x at least; a zero row and a row of +-the bf16 maximum;
    nothing written past [M, K]."""
    big = torch.finfo(torch.bfloat16).max
    for M in (1, 3, 64, 257):
        base = _bf(M, K + 64)
        base *= torch.exp2((torch.arange(M, device=DEV) % 8 - 4).float())[:, None].to(torch.bfloat16)
        if M > 1:
            base[1] = 0
        if M > 2:
            base[2, ::2] = big
            base[2, 1::2] = -big
        for x in (base[:, :K].contiguous(), base[:, :K]):
            want_q, want_s = ops.quant_rows_fp8_ref(x.cpu())
            qbuf = torch.full(((M + 1) * K,), 0x7F, dtype=torch.uint8, device=DEV)       # e4m3 NaN
            sbuf = torch.full((M + 1,), float("nan"), device=DEV)
            q, sx = qbuf.view(F8).view(M + 1, K)[:M], sbuf[:M]
            torch.ops.dgi.quant_rows_fp8(q, sx, x)
            assert torch.equal(sx.view(torch.int32).cpu(), want_s.view(torch.int32)), (M, K)
            assert torch.equal(q.view(torch.uint8).cpu(), want_q.view(torch.uint8)), (M, K)
            assert bool((qbuf[M * K:] == 0x7F).all()) and bool(torch.isnan(sbuf[M:]).all())
            # through ops
            q2, s2 = ops.quant_rows_fp8(x)
            assert torch.equal(q2.view(torch.uint8), q.view(torch.uint8)) and torch.equal(s2, sx)
        if M > 2:
            assert float(sx[1]) == 1.0 and not q[1].view(torch.uint8).any()
            assert set(q[2].view(torch.uint8).unique().tolist()) == {0x7E, 0xFE}          # +-448


def test_quant_rows_fp8_rejects_bad_operands():
    x = _bf(4, 64)
    q = torch.zeros(4, 64, dtype=torch.uint8, device=DEV).view(F8)
    sx = torch.zeros(4, device=DEV)
    for bad in (lambda: torch.ops.dgi.quant_rows_fp8(q, sx, _bf(4, 72)[:, :56]),            # K % 16
                lambda: torch.ops.dgi.quant_rows_fp8(q, sx[:3], x),
                lambda: torch.ops.dgi.quant_rows_fp8(q.view(torch.uint8), sx, x),
                lambda: torch.ops.dgi.quant_rows_fp8(q, sx, x.float())):
        with pytest.raises(RuntimeError):
            bad()
    assert not q.view(torch.uint8).any() and not sx.any()


# ---------------------------------------------------------------------------- GEMM, exact

def _int_operands(M, N, K):
    m = torch.arange(M, device=DEV)[:, None]
    n = torch.arange(N, device=DEV)[:, None]
    k = torch.arange(K, device=DEV)[None, :]
    xq = (((3 * m + 5 * k) % 17) - 8).float()
    wq = (((7 * n + 11 * k) % 13) - 6).float()
    sx = torch.exp2((torch.arange(M, device=DEV) % 5 - 2).float())
    sw = torch.exp2((torch.arange(N, device=DEV) % 7 - 3).float())
    return xq, wq, sx, sw


@pytest.mark.parametrize("K", [128, 256, 384, 2048])    # one K tile, both stages, an odd count, steady state
@pytest.mark.parametrize("N", [256, 1280])              # one tile; 5 tiles: the remainder branch of the XCD map
def test_mfma_gemm_fp8_exact_integers(N, K):
    """Small-integer operands (exact in e4m3, every partial sum an integer below 2^24) and
    power-of-two scales: the result is exact whatever the summation order, so a fragment that
    pairs the wrong k, a row or column in the wrong place, a wrong scale or a missed tile shows
    as an unequal bit."""
    for M in (1, 33, 255, 256, 257, 300):               # the clamped tail, an exact tile, one row into a second
        xq, wq, sx, sw = _int_operands(M, N, K)
        ref = (xq.double() @ wq.double().T).float()
        assert bool((ref.abs() < 2 ** 24).all())
        got = _gemm(xq.to(F8), sx, wq.to(F8), sw)
        assert torch.equal(got, (ref * sx[:, None] * sw[None, :]).to(torch.bfloat16)), (M, N, K)
        bias = ((torch.arange(N, device=DEV) % 9) - 4).to(torch.bfloat16)
        got = _gemm(xq.to(F8), sx, wq.to(F8), sw, bias)
        assert torch.equal(got, (ref * sx[:, None] * sw[None, :] + bias.float()).to(torch.bfloat16)), (M, N, K)


@pytest.mark.parametrize("M,N,K", [(300, 1280, 384), (40, 256, 2048)])
def test_mfma_gemm_fp8_one_hot(M, N, K):
    """A = I-like: row m of Xq is one-hot at k(m), so out[m, n] = Wq[n, k(m)] * sx[m] * sw[n] — a
    swapped row / column store or a transposed block cannot pass against the asymmetric Wq."""
    _, wq, sx, sw = _int_operands(M, N, K)
    km = (torch.arange(M, device=DEV) * 37 + 5) % K
    xq = torch.zeros(M, K, device=DEV)
    xq[torch.arange(M, device=DEV), km] = 1.0
    got = _gemm(xq.to(F8), sx, wq.to(F8), sw)
    want = (wq[:, km].T * sx[:, None] * sw[None, :]).to(torch.bfloat16)
    assert torch.equal(got, want)


def _check(got, ref, S, what):
    """|got - ref| <= 2^-8 |ref| + 2^-10 S with S = (sum_k |xq||wq|) sx sw (+ |bias|): one bf16
    rounding with a factor 2 of slack, plus the worst-case fp32 sequential-sum bound K 2^-24 S
    at K = 16384."""
    err = (got.double() - ref.double()).abs()
    bound = 2.0 ** -8 * ref.double().abs() + 2.0 ** -10 * S.double()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: worst error / bound = {worst:.4f}")
    assert bool((err <= bound).all()), (what, worst)


@pytest.mark.parametrize("M", [40, 256])
def test_mfma_gemm_fp8_every_code(M):
    """All 254 finite e4m3 codes on both sides in every lane position: an fnuz decode, a dropped
    subnormal, a sign error or a wrong scale byte misses the bound by orders of magnitude."""
    fw = _every_code()
    xq = _codes(M, 1024, 5, 3)
    sx = torch.exp2((torch.arange(M, device=DEV) % 5 - 2).float())
    got = _gemm(xq, sx, fw.q, fw.scale)
    xd, wd = xq.float().double(), fw.q.float().double()
    ref = (xd @ wd.T) * sx[:, None].double()
    S = (xd.abs() @ wd.abs().T) * sx[:, None].double()
    _check(got, ref, S, f"every code M={M}")


@pytest.mark.parametrize("M,N,K", [(300, 1280, 2048), (64, 256, 14336), (1, 512, 1024)])
def test_linear_w8a8_random(M, N, K):
    fw = _weight(N, K)
    b = _bf(N)
    for x in (_bf(M, K), _bf(M, K + 64)[:, :K]):
        q, sx = ops.quant_rows_fp8(x)
        qr, sr = ops.quant_rows_fp8_ref(x.cpu())
        assert torch.equal(q.view(torch.uint8).cpu(), qr.view(torch.uint8)) and torch.equal(sx.cpu(), sr)
        S0 = ((q.float().double().abs() @ fw.q.float().double().abs().T) * sx[:, None].double()
              * fw.scale[None, :].double())
        for bias in (None, b):
            ref = ops.linear_w8a8_ref(x.float(), fw, bias)          # fp32, not rounded to bf16
            S = S0 if bias is None else S0 + bias.double().abs()
            got = ops.linear_w8a8(x, fw, bias)
            assert got.dtype == torch.bfloat16 and got.shape == (M, N)
            _check(got, ref, S, f"random {M}x{N}x{K} bias={bias is not None}")
            out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
            assert ops.linear_w8a8(x, fw, bias, out) is out and torch.equal(out, got)
            wide = torch.full((M, N + 8), float("nan"), dtype=torch.bfloat16, device=DEV)     # strided out
            assert ops.linear_w8a8(x, fw, bias, wide[:, :N]).data_ptr() == wide.data_ptr()
            assert torch.equal(wide[:, :N], got) and bool(torch.isnan(wide[:, N:]).all())


def test_mfma_gemm_fp8_rejects_bad_operands():
    M = 40

    def run(N, K, sx_n=None, wq_dtype=None):
        xq = torch.zeros(M, K, dtype=torch.uint8, device=DEV).view(F8)
        wq = torch.zeros(N, K, dtype=torch.uint8, device=DEV)
        wq = wq if wq_dtype is torch.uint8 else wq.view(F8)
        out = torch.full((M, N), 7.0, dtype=torch.bfloat16, device=DEV)
        with pytest.raises(RuntimeError):
            torch.ops.dgi.mfma_gemm_fp8(out, xq, torch.ones(sx_n or M, device=DEV), wq, torch.ones(N, device=DEV), None)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())
    run(128, 256)
    run(256, 192)
    run(256, 256, sx_n=M - 1)
    run(256, 256, wq_dtype=torch.uint8)


def test_mfma_gemm_fp8_misaligned_codes():
    """A contiguous e4m3 view at a 1-byte storage offset: the op refuses it (16-byte loads) and
    ``ops`` routes it away from the kernels."""
    M, N, K = 40, 256, 256
    buf = torch.zeros(N * K + 16, dtype=torch.uint8, device=DEV)
    wq = buf[1:1 + N * K].view(F8).view(N, K)
    assert wq.is_contiguous() and wq.data_ptr() % 16 == 1
    xq = torch.zeros(M, K, dtype=torch.uint8, device=DEV).view(F8)
    out = torch.full((M, N), 7.0, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError):
        torch.ops.dgi.mfma_gemm_fp8(out, xq, torch.ones(M, device=DEV), wq, torch.ones(N, device=DEV), None)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    fw = Fp8Weight(wq, torch.ones(N, device=DEV), act="fp8")
    x = _bf(M, K)
    assert not ops._w8a8_fits(x, fw)
    assert ops._w8a8_fits(x, Fp8Weight(buf[:N * K].view(F8).view(N, K), fw.scale, act="fp8"))


# ---------------------------------------------------------------------------- routing

def test_linear_routing_w8a8(monkeypatch):
    monkeypatch.setattr(ops, "W8A8_MIN_M", 33)
    names = _spy(monkeypatch)
    fw = quantize_fp8(_bf(1280, 2048, scale=0.05))
    fa = Fp8Weight(fw.q, fw.scale, act="fp8")
    b = _bf(1280)
    for M in (33, 300):
        del names[:]
        x = _bf(M, 2048)
        got = ops.linear(x, fa, b)
        assert names == ["quant_rows_fp8", "mfma_gemm_fp8"]
        assert torch.equal(got, ops.linear_w8a8(x, fa, b))
    del names[:]
    x = _bf(8, 2048)
    got = ops.linear(x, fa, b)
    assert names == ["skinny_gemm_w8"]
    assert torch.equal(got, ops.linear(x, fw, b))
    # N not a multiple of 256: today's dequant route
    del names[:]
    f35 = quantize_fp8(_bf(1152, 3584, scale=0.05))
    f35a = Fp8Weight(f35.q, f35.scale, act="fp8")
    x = _bf(40, 3584)
    got = ops.linear(x, f35a)
    assert names == ["dequant_fp8"]
    assert torch.equal(got, ops.linear(x, f35))


def test_linear_routing_act_none_unchanged(monkeypatch):
    """The op names of test_fp8_weights_gpu.test_linear_routing's cases, with act left at None."""
    names = _spy(monkeypatch)
    fw = quantize_fp8(_bf(1152, 2048, scale=0.05))
    assert fw.act is None
    b = _bf(1152)
    ref = lambda x, w, bias=None: (x.float() @ (w.q.float() * w.scale[:, None]).t()    # noqa: E731
                                   + (0 if bias is None else bias.float()))
    for M in (33, 300):
        x = _bf(M, 2048)
        torch.testing.assert_close(ops.linear(x, fw, b).float(), ref(x, fw, b), **TOL)
    fw35 = quantize_fp8(_bf(1152, 3584, scale=0.05))
    x = _bf(1, 3584)
    torch.testing.assert_close(ops.linear(x, fw35).float(), ref(x, fw35), **TOL)
    assert names == ["dequant_fp8"] * 3
    del names[:]
    x = _bf(8, 2048)
    torch.testing.assert_close(ops.linear(x, fw, b).float(), ref(x, fw, b), **TOL)
    fwl = quantize_fp8(_bf(256, 14336, scale=0.05))
    x = _bf(32, 14336)
    torch.testing.assert_close(ops.linear(x, fwl).float(), ref(x, fwl), **TOL)
    # a shape the e4m3 GEMM takes still dequantises without the knob
    assert ops.linear(_bf(64, 14336), fwl).shape == (64, 256)
    assert names == ["skinny_gemm_w8", "skinny_gemm_w8", "dequant_fp8"]


# ---------------------------------------------------------------------------- engine

def _teacher_forced_ok(name, f32_model, prompts, gpu_outs, rel=0.03, abs_=0.02):
    """Every token the GPU chose is an argmax of the fp32 CPU model's logits for the same prefix
    (teacher forced), up to a bf16 tolerance — per step, every prompt (as in test_fp8_weights_gpu)."""
    from dgi.engine import EngineConfig, LLMEngine
    from dgi.sched.request import SamplingParams
    ref = LLMEngine(EngineConfig(model=name, device="cpu", dtype=torch.float32, num_blocks=256, max_num_seqs=8,
                                 max_model_len=512, max_num_batched_tokens=256, use_graphs=False,
                                 enable_prefix_caching=False, weight_quant=f32_model.weight_quant,
                                 act_quant=f32_model.act_quant), model_cfg=f32_model.cfg, model=f32_model)
    got = {}
    orig = ref.model.compute_logits

    def spy(h, residual, idx):
        out = orig(h, residual, idx)
        got["l"] = out[-1].detach().float()
        return out
    ref.model.compute_logits = spy
    one = SamplingParams(max_tokens=1, temperature=0.0, ignore_eos=True)
    checked, worst = 0, 0.0
    for p, toks in zip(prompts, gpu_outs):
        for t, tok in enumerate(toks):
            ref.generate([p + toks[:t]], one)
            r = got["l"]
            worst = max(worst, float(r.max() - r[tok]) / float(r.abs().max()))
            tol = rel * float(r.abs().max()) + abs_
            assert float(r[tok]) >= float(r.max()) - tol, (name, len(p), t, tok, int(r.argmax()))
            checked += 1
    print(f"teacher forced: worst (max logit - chosen logit) / max|logit| = {worst:.5f}")
    return checked


def _engine(mc, src, graphs):
    from dgi.engine import EngineConfig, LLMEngine
    from dgi.models.llama import LlamaModel
    gm = LlamaModel(mc, "cuda", init="empty").copy_from(src)
    eng = LLMEngine(EngineConfig(model=mc.name, device="cuda", num_blocks=256, max_num_seqs=8, max_model_len=512,
                                 max_num_batched_tokens=256, use_graphs=graphs, weight_quant="fp8",
                                 act_quant="fp8"), model_cfg=mc, model=gm)
    assert gm.weight_quant == "fp8" and gm.act_quant == "fp8"
    return eng, gm


def test_w8a8_engine_teacher_forced(monkeypatch):
    """llama-tiny-hd128 with every projection of every step W8A8 (threshold 1), eager and graph-replayed:
    all 40 tokens against an fp32 CPU model holding the same codes and emulating the quantiser."""
    from dgi.models.config import get_config
    from dgi.models.llama import LlamaModel
    from dgi.sched.request import SamplingParams
    monkeypatch.setattr(ops, "W8A8_MIN_M", 1)
    name = "llama-tiny-hd128"
    mc = get_config(name)
    src = LlamaModel(mc, "cpu", seed=5)
    sp = SamplingParams(max_tokens=10, temperature=0.0, ignore_eos=True)
    names = _spy(monkeypatch)
    outs, models = {}, {}
    for graphs in (False, True):
        eng, gm = _engine(mc, src, graphs)
        del names[:]
        outs[graphs] = [r.output for r in eng.generate(PROMPTS, sp)]
        assert "mfma_gemm_fp8" in names and "quant_rows_fp8" in names
        assert not {"dequant_fp8", "skinny_gemm_w8", "mfma_gemm", "fused_skinny"} & set(names)
        models[graphs] = gm
    assert all(len(o) == 10 for o in outs[False])
    f32 = LlamaModel(mc, "cpu", torch.float32, init="empty").copy_from(src)
    f32.quantize_weights("fp8", act_quant="fp8").copy_from(models[False])
    assert torch.equal(f32.layers[1].down.q.view(torch.uint8), models[False].layers[1].down.q.view(torch.uint8).cpu())
    assert _teacher_forced_ok(name, f32, PROMPTS, outs[False]) == 40
    # fixed reduction order: the graph replay computes the same tokens
    assert outs[True] == outs[False]


def test_w8a8_engine_default_threshold(monkeypatch):
    """Threshold 33 (every step the W8A16 kernel does not take), graphs on: prefill chunks take the e4m3 GEMM, decode steps the W8A16 kernel,
    and nothing is dequantised."""
    from dgi.models.config import get_config
    from dgi.models.llama import LlamaModel
    from dgi.sched.request import SamplingParams
    monkeypatch.setattr(ops, "W8A8_MIN_M", 33)
    mc = get_config("llama-tiny-hd128")
    src = LlamaModel(mc, "cpu", seed=5)
    names = _spy(monkeypatch)
    eng, _gm = _engine(mc, src, True)
    del names[:]
    outs = [r.output for r in eng.generate(PROMPTS, SamplingParams(max_tokens=10, temperature=0.0, ignore_eos=True))]
    assert all(len(o) == 10 for o in outs)
    assert "mfma_gemm_fp8" in names and "skinny_gemm_w8" in names and "dequant_fp8" not in names
