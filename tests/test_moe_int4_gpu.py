"""INT4 weight-only experts on the GPU: ``moe_gemm_w4`` (dgi/csrc/moe_int4.hip) against exact answers and a float64
product with ``dequant()``, ``ops.moe_mlp`` eager and in a graph, and the ``qwen3-moe-tiny`` engine with
``expert_quant="awq"`` (the CPU side: tests/test_moe_int4.py)."""
import pytest
import torch

import test_moe_gpu as moe_gpu
from dgi import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
GEMM_ATOL, GEMM_RTOL = 3e-2, 2e-2      # the skinny GEMM's bound, as tests/test_moe_gpu.py uses
_launches, _nan_like = moe_gpu._launches, moe_gpu._nan_like


@pytest.fixture(autouse=True, scope="module")
def _native():
    ops.load_native(required=True)


def _gpu(iw):
    return ops.Int4ExpertWeight(iw.q.to(DEV), iw.sz.to(DEV))


def _ids(T, k, E, g):
    return torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(T)]).to(torch.int32)


def _gemm(x_tok, iw, ids, epi, BM):
    """``moe_gemm`` over the layout of ``ids`` [T, k], per slot.  SwiGLU gathers ``x_tok``; plain reads slot s's
    token row s // k in sorted order, x's padding rows NaN.  ``out`` starts as NaN and its padding rows stay so."""
    k, N = ids.shape[1], iw.shape[1] // 2 if epi else iw.shape[1]
    _c, _o, sorted_slot, block_expert, inv = ops.moe_align(ids.to(DEV), iw.shape[0], BM)
    x = x_tok.to(DEV)
    if not epi:
        x = _nan_like(sorted_slot.numel(), x_tok.shape[1])
        x[inv.long()] = x_tok.to(DEV).repeat_interleave(k, 0)
    out = ops.moe_gemm(x, _gpu(iw), sorted_slot, block_expert, k, epi, BM, out=_nan_like(sorted_slot.numel(), N))
    assert int((sorted_slot < 0).sum()) > 0 and torch.isnan(out[sorted_slot < 0].float()).all()
    return out[inv.long()].cpu()


def _ref64(x_tok, iw, ids, epi):
    w, k = iw.dequant(torch.float64), ids.shape[1]
    y = torch.stack([x_tok[s // k].double() @ w[e].t() for s, e in enumerate(ids.flatten().tolist())])
    return torch.nn.functional.silu(y[:, :y.shape[1] // 2]) * y[:, y.shape[1] // 2:] if epi else y


def _worst(out, ref):
    return float(((out - ref).abs() / (GEMM_ATOL + GEMM_RTOL * ref.abs())).max())


@pytest.mark.parametrize("BM", [16, 32])
@pytest.mark.parametrize("N", [512, 2048])
@pytest.mark.parametrize("K", [256, 512, 768, 2048])
@pytest.mark.parametrize("epi", [0, 1])
def test_moe_gemm_w4_exact(epi, K, N, BM, monkeypatch):
    """Codes 0..15, zero points 7..9 and fp16 scales 0.5 / 1 / 2 that differ between neighbouring groups, rows, experts
    and gate / up (rows n and N + n, N % 3 != 0), x in {-1, 0, 1}: every group sum, fold and cross-wave sum is exact
    in fp32.  K = 256: one step per wave; 512, 2048: four waves; 768: three groups per wave in a depth-2 ring.
    Plain: experts with 0, 1, 16, 17 and 33 rows, bit for bit.  SwiGLU (k = 2): silu is held to the GEMM bound."""
    g = torch.Generator().manual_seed(K + N + BM + epi)
    E, rows = (6, 2 * N) if epi else (5, N)
    e, n, h = torch.meshgrid(torch.arange(E), torch.arange(rows), torch.arange(K // 128), indexing="ij")
    scale, zero = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float16)[(e + n + h) % 3], 7 + (e + 2 * n + h) % 3
    code = torch.randint(0, 16, (E, rows, K), generator=g)
    one = [ops.Int4Weight.pack(code[i], zero[i], scale[i]) for i in range(E)]
    iw = ops.Int4ExpertWeight(torch.stack([o.q for o in one]), torch.stack([o.sz for o in one]))
    if epi:
        ids = _ids(21, 2, E, g)
    else:
        ids = torch.cat([torch.full((c,), i, dtype=torch.int32) for i, c in enumerate([0, 1, 16, 17, 33])])
        ids = ids[torch.randperm(ids.numel(), generator=g)].reshape(-1, 1)
    x = torch.randint(-1, 2, (ids.shape[0], K), generator=g).bfloat16()
    names = _launches(monkeypatch)
    out, ref = _gemm(x, iw, ids, epi, BM), _ref64(x, iw, ids, epi)
    assert names.count("moe_gemm_w4") == 1 and float(ref.abs().max()) > (0.5 if epi else 64)
    if epi:
        torch.testing.assert_close(out.double(), ref, atol=GEMM_ATOL, rtol=GEMM_RTOL)
    else:
        assert torch.equal(out, ref.float().bfloat16())


@pytest.mark.parametrize("T,k,E,K,N,BM,epi", [(7, 4, 8, 2048, 768, 16, 1), (45, 2, 5, 2048, 768, 32, 1),
                                              (9, 4, 8, 768, 2048, 16, 0), (50, 2, 5, 768, 2048, 32, 0)])
def test_moe_gemm_w4_random(T, k, E, K, N, BM, epi, monkeypatch):
    g = torch.Generator().manual_seed(T + K)
    ids, x = _ids(T, k, E, g), torch.randn(T, K, generator=g).bfloat16()
    iw = ops.quantize_int4_experts((torch.randn(E, 2 * N if epi else N, K, generator=g) / K ** 0.5).bfloat16())
    names = _launches(monkeypatch)
    out, ref = _gemm(x, iw, ids, epi, BM).double(), _ref64(x, iw, ids, epi)
    assert names.count("moe_gemm_w4") == 1 and float(ref.abs().max()) > 0.5
    print(f"moe_gemm_w4 epi={epi} T={T} K={K} N={N} BM={BM}: worst error / bound = {_worst(out, ref):.3f}")
    torch.testing.assert_close(out, ref, atol=GEMM_ATOL, rtol=GEMM_RTOL)


@pytest.mark.parametrize("epi", [0, 1])
@pytest.mark.parametrize("K", [768, 512, 2048])
def test_moe_gemm_w4_rows_do_not_depend_on_the_row_block(K, epi):
    """The same slots at BM = 16 and BM = 32 are bit-equal: step depth and wave count are functions of K alone."""
    g = torch.Generator().manual_seed(K)
    ids, x = _ids(37, 2, 4, g), torch.randn(37, K, generator=g).bfloat16()
    iw = ops.quantize_int4_experts(torch.randn(4, 256 if epi else 128, K, generator=g) / K ** 0.5)
    a, b = _gemm(x, iw, ids, epi, 16), _gemm(x, iw, ids, epi, 32)
    assert torch.isfinite(a.float()).all() and float(a.float().abs().max()) > 0.5 and torch.equal(a, b)


@pytest.mark.parametrize("E,k,H,I,Ts", [(8, 2, 512, 256, (1, 17, 300)), (128, 8, 2048, 768, (1, 40))])
def test_moe_mlp_int4_experts(E, k, H, I, Ts, monkeypatch):
    router, gate_up, down, make_x = moe_gpu._mlp_weights(E, H, I, seed=E)
    gate_up, down = ops.quantize_int4_experts(gate_up), ops.quantize_int4_experts(down)
    assert gate_up.q.is_cuda and ops.moe_mlp_ok(make_x(1), router, gate_up, down, k)
    names = _launches(monkeypatch)
    with torch.inference_mode():
        for T in Ts:
            x = make_x(T)
            names.clear()
            out = ops.moe_mlp(x, router, gate_up, down, k, True)
            assert [n for n in names if n.startswith("moe_")] == ["moe_route", "moe_align", "moe_gemm_w4", "moe_gemm_w4",
                                                                   "moe_combine"]
            ids, _ = ops.moe_route(ops.linear(x, router), k, True)
            ref = ops.moe_mlp_ref(x, router, gate_up, down, k, True, ids=ids).float()   # per expert, the same container
            assert float(ref.abs().max()) > 0.05
            print(f"moe_mlp int4 experts E={E} H={H} I={I} T={T}: worst error / bound = {_worst(out.float(), ref):.3f}")
            torch.testing.assert_close(out.float(), ref, atol=GEMM_ATOL, rtol=GEMM_RTOL)
            static = x.clone()                                      # one capture, replayed on new and old rows
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                ops.moe_mlp(static, router, gate_up, down, k, True)
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                held = ops.moe_mlp(static, router, gate_up, down, k, True)
            for x2 in (make_x(T), x, x):
                static.copy_(x2)
                graph.replay()
                torch.cuda.synchronize()
                assert torch.equal(held, ops.moe_mlp(x2, router, gate_up, down, k, True)), T
            assert torch.equal(held, out)
            del graph


def test_refusals_take_the_reference_and_never_launch(monkeypatch):
    g = torch.Generator().manual_seed(0)
    _c, _o, sorted_slot, block_expert, _inv = ops.moe_align(_ids(6, 2, 4, g).to(DEV), 4, 16)
    w384 = ops.quantize_int4_experts(torch.randn(4, 64, 384, generator=g) / 16)
    w256 = ops.quantize_int4_experts(torch.randn(4, 64, 256, generator=g) / 16)
    x384, x256 = torch.randn(6, 384, generator=g).bfloat16().to(DEV), torch.randn(6, 256, generator=g).bfloat16().to(DEV)
    names = _launches(monkeypatch)
    for x, w, lay in ((x384, _gpu(w384), (sorted_slot, block_expert)),          # K % 256 != 0
                      (x256.half(), _gpu(w256), (sorted_slot, block_expert)),   # fp16 x
                      (x256.cpu(), w256, (sorted_slot.cpu(), block_expert.cpu()))):     # a CPU container
        out = ops.moe_gemm(x, w, *lay, 2, ops.MOE_EPI_SWIGLU, 16)
        assert torch.equal(out, ops.moe_gemm_ref(x, w, *lay, 2, ops.MOE_EPI_SWIGLU, 16))
    assert names == []
    gw, mk_out = _gpu(w256), lambda: torch.empty(sorted_slot.numel(), 32, dtype=torch.bfloat16, device=DEV)
    torch.ops.dgi.moe_gemm_w4(mk_out(), x256, gw.q, gw.sz, sorted_slot, block_expert, 2, 12, 1, 16)   # the good call
    for q, sz in ((_gpu(w384).q, _gpu(w384).sz), (gw.q, gw.sz[:, :, :1].contiguous()), (gw.q.float(), gw.sz)):
        with pytest.raises(RuntimeError):
            torch.ops.dgi.moe_gemm_w4(mk_out(), x256, q, sz, sorted_slot, block_expert, 2, 12, 1, 16)
    torch.cuda.synchronize()


def test_moe_engine_int4_experts_gpu(monkeypatch):
    """qwen3-moe-tiny with ``expert_quant="awq"``: graphs == eager, run to run, and every token is within
    ``0.03 max|ref| + 0.02`` of the maximum of the fp32 CPU model that holds the dequantised experts, with the routing
    the GPU recorded."""
    from dgi.engine import EngineConfig, LLMEngine
    from dgi.models.config import get_config
    from dgi.models.llama import EXPERT_SLOTS, LlamaModel
    from dgi.sched.request import SamplingParams
    name = "qwen3-moe-tiny"
    mc = get_config(name)
    cpu_model = LlamaModel(mc, "cpu", seed=5)
    prompts = [[1] + list(range(7, 7 + n - 1)) for n in (3, 60, 300)]
    sp = SamplingParams(max_tokens=10, temperature=0.0, ignore_eos=True)
    gm = LlamaModel(mc, "cuda", init="empty").copy_from(cpu_model)
    names = _launches(monkeypatch)
    engine = lambda graphs: LLMEngine(EngineConfig(                   # noqa: E731
        model=name, device="cuda", num_blocks=128, max_num_seqs=4, max_model_len=512, max_num_batched_tokens=512,
        use_graphs=graphs, enable_prefix_caching=False, expert_quant="awq"), model_cfg=mc, model=gm)
    eager_eng = engine(False)
    assert gm.expert_quant == "int4" and isinstance(gm.layers[0].experts_down, ops.Int4ExpertWeight)
    assert gm.layers[0].qkv.dtype == torch.bfloat16 and gm.layers[0].router.dtype == torch.bfloat16
    eager = [r.output for r in eager_eng.generate(prompts, sp)]
    assert "moe_gemm_w4" in names and "moe_gemm" not in names and "moe_gemm_w8" not in names
    rec_outs, records = moe_gpu._recorded_run(eager_eng, prompts, sp)
    f32 = LlamaModel(mc, "cpu", torch.float32, init="empty").copy_from(cpu_model)
    for L, Lg in zip(f32.layers, gm.layers):
        for k in EXPERT_SLOTS:
            getattr(L, k).copy_(getattr(Lg, k).dequant(torch.float32))
    assert moe_gpu._teacher_forced_ok(name, f32, prompts, rec_outs, records) == 30
    assert [r.output for r in eager_eng.generate(prompts, sp)] == eager          # run to run
    graph_eng = engine(True)
    assert [r.output for r in graph_eng.generate(prompts, sp)] == eager
    assert [r.output for r in graph_eng.generate(prompts, sp)] == eager          # and again
