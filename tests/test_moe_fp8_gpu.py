"""FP8 weight-only experts on the GPU: ``moe_gemm_w8`` (dgi/csrc/moe.hip over ``E4m3W``) against
exact answers and against ``moe_gemm_ref`` on the container, ``ops.moe_mlp`` with quantised experts
eager and in a graph, and the engine on ``qwen3-moe-tiny`` with ``expert_quant="fp8"`` (the CPU side:
tests/test_moe_fp8.py)."""
import pytest
import torch

import test_moe_gpu as moe_gpu
from dgi import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
GEMM_ATOL, GEMM_RTOL = 3e-2, 2e-2      # the skinny GEMM's bound, as tests/test_fp8_weights_gpu.py uses
_launches, _nan_like, _random_layout = moe_gpu._launches, moe_gpu._nan_like, moe_gpu._random_layout


@pytest.fixture(autouse=True, scope="module")
def _native():
    ops.load_native(required=True)


# ---------------------------------------------------------------------------- moe_gemm_w8: exact answers

def _exact_operands(E, rows, K, g):
    """Codes in {-2 .. 2} (exact in e4m3) and per-channel scales in {0.5, 1, 2} that differ between
    neighbouring channels and between experts: every product, sum and scaling is exact in fp32."""
    codes = torch.randint(-2, 3, (E, rows, K), generator=g).float()
    e_i, n_i = torch.meshgrid(torch.arange(E), torch.arange(rows), indexing="ij")
    scale = torch.tensor([0.5, 1.0, 2.0])[(n_i + e_i) % 3].contiguous()
    assert not torch.equal(scale[:, 1:], scale[:, :-1]) and not torch.equal(scale[1:], scale[:-1])
    return codes, scale


def _container(codes, scale):
    return ops.Fp8ExpertWeight(codes.to(torch.float8_e4m3fn).to(DEV), scale.to(DEV))


def _exact_plain(counts, K, N, BM, seed):
    g = torch.Generator().manual_seed(seed)
    E = len(counts)
    ids = torch.cat([torch.full((c,), e, dtype=torch.int32) for e, c in enumerate(counts)])
    ids = ids[torch.randperm(ids.numel(), generator=g)].reshape(-1, 1)          # k = 1: slot = token
    _c, _o, sorted_slot, block_expert, inv = ops.moe_align(ids.to(DEV), E, BM)
    P = sorted_slot.numel()
    codes, scale = _exact_operands(E, N, K, g)
    fw = _container(codes, scale)
    assert torch.equal(fw.q.float().cpu(), codes)
    xt = torch.randint(-1, 2, (ids.numel(), K), generator=g).bfloat16()
    xs = _nan_like(P, K)
    xs[inv.long()] = xt.to(DEV)
    out = _nan_like(P, N)
    ops.moe_gemm(xs, fw, sorted_slot, block_expert, 1, ops.MOE_EPI_PLAIN, BM, out=out)
    out = out.cpu()
    real = sorted_slot.cpu() >= 0
    assert torch.isfinite(out[real].float()).all() and torch.isnan(out[~real].float()).all()
    ref = torch.stack([(xt[t].float() @ codes[int(ids[t, 0])].t()) * scale[int(ids[t, 0])]
                       for t in range(ids.numel())]).bfloat16()
    assert torch.equal(out[inv.cpu().long()], ref)
    assert float(ref.float().abs().max()) > 8


@pytest.mark.parametrize("BM", [16, 32])
@pytest.mark.parametrize("K,N", [(256, 512), (768, 2048), (768, 512), (512, 2048)])
def test_moe_gemm_w8_exact_plain(K, N, BM, monkeypatch):
    """K = 256 and 768 take the 2-wave geometry, K = 512 the 4-wave one."""
    names = _launches(monkeypatch)
    _exact_plain([0, 1, 15, 16, 17, 33], K, N, BM, seed=K + N)
    _exact_plain([0, 0, 40, 0], K, N, BM, seed=K + N + 1)                      # every row in one expert
    assert names.count("moe_gemm_w8") == 2 and "moe_gemm" not in names


@pytest.mark.parametrize("BM", [16, 32])
@pytest.mark.parametrize("K,N", [(256, 512), (768, 2048), (768, 512), (512, 2048)])
def test_moe_gemm_w8_exact_swiglu(K, N, BM, monkeypatch):
    """The same operands through the SwiGLU gather with k = 2.  Gate scales differ from up scales (row
    n of gate and row N + n of up: N % 3 != 0), token rows are distinct at O(1)."""
    g = torch.Generator().manual_seed(K + N + BM)
    names = _launches(monkeypatch)
    T, k, E = 21, 2, 6
    ids, (_c, _o, sorted_slot, block_expert, inv) = _random_layout(T, k, E, BM, g)
    codes, scale = _exact_operands(E, 2 * N, K, g)
    assert not torch.equal(scale[:, :N], scale[:, N:])
    fw = _container(codes, scale)
    x = torch.randint(-1, 2, (T, K), generator=g).bfloat16()
    assert torch.unique(x, dim=0).shape[0] == T
    out = _nan_like(sorted_slot.numel(), N)
    ops.moe_gemm(x.to(DEV), fw, sorted_slot, block_expert, k, ops.MOE_EPI_SWIGLU, BM, out=out)
    assert names.count("moe_gemm_w8") == 1
    ref = ops.moe_gemm_ref(x, ops.Fp8ExpertWeight(fw.q.cpu(), fw.scale.cpu()), sorted_slot.cpu(), block_expert.cpu(), k,
                           ops.MOE_EPI_SWIGLU, BM,
                           out=torch.full((sorted_slot.numel(), N), float("nan"), dtype=torch.bfloat16))
    out = out.cpu()
    real = sorted_slot.cpu() >= 0
    assert int(real.sum()) == T * k and torch.isnan(out[~real].float()).all() and torch.isnan(ref[~real].float()).all()
    assert float(ref[real].float().abs().max()) > 0.5
    torch.testing.assert_close(out[real].float(), ref[real].float(), atol=GEMM_ATOL, rtol=GEMM_RTOL)


# ---------------------------------------------------------------------------- moe_gemm_w8: random operands

def _worst(out, ref):
    """max over elements of |out - ref| / (atol + rtol |ref|): <= 1 passes assert_close."""
    return float(((out - ref).abs() / (GEMM_ATOL + GEMM_RTOL * ref.abs())).max())


@pytest.mark.parametrize("T,k,E,K,N,BM", [(7, 4, 8, 2048, 768, 16), (45, 2, 5, 2048, 768, 32)])
def test_moe_gemm_w8_swiglu_random(T, k, E, K, N, BM, monkeypatch):
    g = torch.Generator().manual_seed(T + K)
    names = _launches(monkeypatch)
    ids, (_c, _o, sorted_slot, block_expert, inv) = _random_layout(T, k, E, BM, g)
    x = torch.randn(T, K, generator=g).bfloat16()
    fw = ops.quantize_fp8_experts((torch.randn(E, 2 * N, K, generator=g) / K ** 0.5).bfloat16())
    gw = ops.Fp8ExpertWeight(fw.q.to(DEV), fw.scale.to(DEV))
    out = _nan_like(sorted_slot.numel(), N)
    ops.moe_gemm(x.to(DEV), gw, sorted_slot, block_expert, k, ops.MOE_EPI_SWIGLU, BM, out=out)
    assert names.count("moe_gemm_w8") == 1
    ref = ops.moe_gemm_ref(x, fw, sorted_slot.cpu(), block_expert.cpu(), k, ops.MOE_EPI_SWIGLU, BM,
                           out=torch.full((sorted_slot.numel(), N), float("nan"), dtype=torch.bfloat16))
    out = out.cpu()
    real = sorted_slot.cpu() >= 0
    assert int(real.sum()) == T * k and torch.isnan(out[~real].float()).all()
    assert float(ref[real].float().abs().max()) > 0.5
    print(f"moe_gemm_w8 swiglu T={T} K={K} N={N} BM={BM}: worst error / bound = "
          f"{_worst(out[real].float(), ref[real].float()):.3f}")
    torch.testing.assert_close(out[real].float(), ref[real].float(), atol=GEMM_ATOL, rtol=GEMM_RTOL)


@pytest.mark.parametrize("T,k,E,K,N,BM", [(9, 4, 8, 768, 2048, 16), (50, 2, 5, 768, 2048, 32)])
def test_moe_gemm_w8_plain_random(T, k, E, K, N, BM, monkeypatch):
    g = torch.Generator().manual_seed(T + K)
    names = _launches(monkeypatch)
    ids, (_c, _o, sorted_slot, block_expert, inv) = _random_layout(T, k, E, BM, g)
    P = sorted_slot.numel()
    xs = torch.randn(P, K, generator=g).bfloat16()
    fw = ops.quantize_fp8_experts((torch.randn(E, N, K, generator=g) / K ** 0.5).bfloat16())
    gw = ops.Fp8ExpertWeight(fw.q.to(DEV), fw.scale.to(DEV))
    out = ops.moe_gemm(xs.to(DEV), gw, sorted_slot, block_expert, k, ops.MOE_EPI_PLAIN, BM).cpu()
    assert names.count("moe_gemm_w8") == 1
    ref = ops.moe_gemm_ref(xs, fw, sorted_slot.cpu(), block_expert.cpu(), k, ops.MOE_EPI_PLAIN, BM)
    real = sorted_slot.cpu() >= 0
    assert float(ref[real].float().abs().max()) > 0.5
    print(f"moe_gemm_w8 plain T={T} K={K} N={N} BM={BM}: worst error / bound = "
          f"{_worst(out[real].float(), ref[real].float()):.3f}")
    torch.testing.assert_close(out[real].float(), ref[real].float(), atol=GEMM_ATOL, rtol=GEMM_RTOL)


@pytest.mark.parametrize("K,N,epi", [(768, 256, 0), (512, 256, 0), (2048, 128, 1), (768, 128, 1)])
def test_moe_gemm_w8_rows_do_not_depend_on_the_row_block(K, N, epi):
    """Identical tokens routed identically: BM = 16 and BM = 32 give bit-equal rows per slot (the
    wave count is a function of K alone)."""
    g = torch.Generator().manual_seed(K + N)
    T, k, E = 37, 2, 4
    ids = torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(T)]).to(torch.int32).to(DEV)
    fw = ops.quantize_fp8_experts((torch.randn(E, 2 * N if epi else N, K, generator=g) / K ** 0.5).bfloat16())
    gw = ops.Fp8ExpertWeight(fw.q.to(DEV), fw.scale.to(DEV))
    xt = torch.randn(T, K, generator=g).bfloat16().to(DEV)
    got = []
    for BM in (16, 32):
        _c, _o, sorted_slot, block_expert, inv = ops.moe_align(ids, E, BM)
        if epi:
            x = xt
        else:                                                       # slot s multiplies token s // k's row
            x = torch.zeros(sorted_slot.numel(), K, dtype=torch.bfloat16, device=DEV)
            x[inv.long()] = xt.repeat_interleave(k, 0)
        out = ops.moe_gemm(x, gw, sorted_slot, block_expert, k, epi, BM)
        got.append(out[inv.long()])
    assert torch.isfinite(got[0].float()).all() and float(got[0].float().abs().max()) > 0.5
    assert torch.equal(got[0], got[1])


# ---------------------------------------------------------------------------- moe_mlp

def _quantised_mlp_weights(E, H, I, seed):
    router, gate_up, down, make_x = moe_gpu._mlp_weights(E, H, I, seed)
    return router, ops.quantize_fp8_experts(gate_up), ops.quantize_fp8_experts(down), gate_up, down, make_x


@pytest.mark.parametrize("E,k,H,I,Ts", [(8, 2, 512, 256, (1, 17, 300)), (128, 8, 2048, 768, (1, 40))])
def test_moe_mlp_quantised_experts(E, k, H, I, Ts, monkeypatch):
    router, gate_up, down, gate_up_bf16, down_bf16, make_x = _quantised_mlp_weights(E, H, I, seed=E)
    assert gate_up.q.is_cuda and ops.moe_mlp_ok(make_x(1), router, gate_up, down, k)
    names = _launches(monkeypatch)
    with torch.inference_mode():
        for T in Ts:
            x = make_x(T)
            names.clear()
            out = ops.moe_mlp(x, router, gate_up, down, k, True)
            assert [n for n in names if n.startswith("moe_")] == ["moe_route", "moe_align", "moe_gemm_w8", "moe_gemm_w8",
                                                                   "moe_combine"]
            assert torch.equal(out, ops.moe_mlp(x, router, gate_up, down, k, True)), T         # bit-reproducible
            ids, _ = ops.moe_route(ops.linear(x, router), k, True)
            forced = ops.moe_mlp(x, router, gate_up, down, k, True, ids=ids)
            ref = ops.moe_mlp_ref(x, router, gate_up, down, k, True, ids=ids)      # per expert, on the same container
            assert float(ref.float().abs().max()) > 0.05
            print(f"moe_mlp fp8 experts E={E} H={H} I={I} T={T}: worst error / bound = "
                  f"{_worst(out.float(), ref.float()):.3f}")
            for got in (out, forced):
                torch.testing.assert_close(got.float(), ref.float(), atol=GEMM_ATOL, rtol=GEMM_RTOL)
            # in a graph: one capture, replayed on new rows
            static = x.clone()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                ops.moe_mlp(static, router, gate_up, down, k, True)
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                held = ops.moe_mlp(static, router, gate_up, down, k, True)
            x2 = make_x(T)
            static.copy_(x2)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(held, ops.moe_mlp(x2, router, gate_up, down, k, True)), T
            del graph
        # one quantised, one bf16: refused
        for a, b in ((gate_up, down_bf16), (gate_up_bf16, down)):
            with pytest.raises(ValueError, match="Fp8ExpertWeight"):
                ops.moe_mlp(make_x(2), router, a, b, k, True)


def test_refusals_take_the_reference_and_never_launch(monkeypatch):
    g = torch.Generator().manual_seed(0)
    names = _launches(monkeypatch)
    ids, (_c, _o, sorted_slot, block_expert, inv) = _random_layout(6, 2, 4, 16, g)
    P = sorted_slot.numel()
    # K % 256 != 0: the reference, nothing launched
    x = torch.randn(6, 320, generator=g).bfloat16().to(DEV)
    fw = ops.quantize_fp8_experts((torch.randn(4, 64, 320, generator=g) / 16).bfloat16().to(DEV))
    names.clear()
    out = ops.moe_gemm(x, fw, sorted_slot, block_expert, 2, ops.MOE_EPI_SWIGLU, 16)
    assert names == []
    assert torch.equal(out, ops.moe_gemm_ref(x, fw, sorted_slot, block_expert, 2, ops.MOE_EPI_SWIGLU, 16))
    mk_out = lambda: torch.empty(P, 32, dtype=torch.bfloat16, device=DEV)       # noqa: E731
    with pytest.raises(RuntimeError):                                          # K = 320
        torch.ops.dgi.moe_gemm_w8(mk_out(), x, fw.q, fw.scale, sorted_slot, block_expert, 2, 12, 1, 16)
    x = torch.randn(6, 256, generator=g).bfloat16().to(DEV)
    ok = ops.quantize_fp8_experts((torch.randn(4, 64, 256, generator=g) / 16).bfloat16().to(DEV))
    torch.ops.dgi.moe_gemm_w8(mk_out(), x, ok.q, ok.scale, sorted_slot, block_expert, 2, 12, 1, 16)   # the good call
    with pytest.raises(RuntimeError):                                          # bf16 q
        torch.ops.dgi.moe_gemm_w8(mk_out(), x, ok.q.to(torch.bfloat16), ok.scale, sorted_slot, block_expert, 2, 12, 1, 16)
    for bad in (ok.scale[:, :32].contiguous(), ok.scale[:3].contiguous(), ok.scale.reshape(-1),
                ok.scale.double()):                                            # scale shape and dtype
        with pytest.raises(RuntimeError):
            torch.ops.dgi.moe_gemm_w8(mk_out(), x, ok.q, bad, sorted_slot, block_expert, 2, 12, 1, 16)
    torch.cuda.synchronize()
    # a whole block the kernels refuse is the reference
    router, gate_up, down, _gb, _db, make_x = _quantised_mlp_weights(4, 320, 256, seed=1)
    xx = make_x(3)
    names.clear()
    out = ops.moe_mlp(xx, router, gate_up, down, 2, True)
    assert not [n for n in names if n.startswith("moe_")]
    assert torch.equal(out, ops.moe_mlp_ref(xx, router, gate_up, down, 2, True))


# ---------------------------------------------------------------------------- engine

def _teacher_forced_ok(name, f32, prompts, gpu_outs, records, rel=0.03, abs_=0.02, kv_dtype=None):
    """tests/test_moe_gpu._teacher_forced_ok for a model the caller built: ``f32`` is the fp32 CPU model
    holding the GPU model's exact codes and scales.  Every token the GPU chose is an argmax of its
    logits for the same prefix up to the tolerance, with the routing the GPU recorded."""
    from dgi.engine import EngineConfig, LLMEngine
    from dgi.sched.request import SamplingParams
    mc = f32.cfg
    kw = {"kv_dtype": kv_dtype} if kv_dtype else {}
    ref = LLMEngine(EngineConfig(model=name, device="cpu", dtype=torch.float32, num_blocks=256, max_num_seqs=8,
                                 max_model_len=512, max_num_batched_tokens=512, use_graphs=False,
                                 enable_prefix_caching=False, expert_quant="fp8", **kw), model_cfg=mc, model=f32)
    got, cur = {}, {}
    orig = ref.model.compute_logits

    def spy(h, residual, idx):
        out = orig(h, residual, idx)
        got["l"] = out[-1].detach().float()
        return out

    def force(layer, positions, ids, weights):
        rows = [cur["rec"].get((layer, p), own) for p, own in zip(positions.tolist(), ids.tolist())]
        return torch.tensor(rows, dtype=torch.int32)
    ref.model.compute_logits = spy
    ref.model.route_hook = force
    one = SamplingParams(max_tokens=1, temperature=0.0, ignore_eos=True)
    checked = 0
    worst = 0.0
    try:
        for p, toks, rec in zip(prompts, gpu_outs, records):
            cur["rec"] = rec
            for t, tok in enumerate(toks):
                ref.generate([p + toks[:t]], one)
                r = got["l"]
                tol = rel * float(r.abs().max()) + abs_
                worst = max(worst, (float(r.max()) - float(r[tok])) / tol)
                assert float(r[tok]) >= float(r.max()) - tol, (name, len(p), t, tok, int(r.argmax()))
                checked += 1
    finally:
        ref.model.compute_logits = orig
        ref.model.route_hook = None
    print(f"{name} expert_quant=fp8 kv={kv_dtype}: {checked} tokens, worst (max - chosen) / tol = {worst:.3f}")
    return checked


@pytest.mark.parametrize("kv_dtype", [None, "fp8"])
def test_moe_engine_fp8_experts_gpu(kv_dtype, monkeypatch):
    """qwen3-moe-tiny with ``expert_quant="fp8"``: graphs == eager, run to run, and every token is within
    ``0.03 max|ref| + 0.02`` of the maximum of an fp32 CPU engine that holds the same codes (``copy_from``)
    with the routing the GPU recorded."""
    from dgi.engine import EngineConfig, LLMEngine
    from dgi.models.config import get_config
    from dgi.models.llama import LlamaModel
    from dgi.sched.request import SamplingParams
    name = "qwen3-moe-tiny"
    mc = get_config(name)
    cpu_model = LlamaModel(mc, "cpu", seed=5)
    prompts = [[1] + list(range(7, 7 + n - 1)) for n in (3, 60, 300)]
    sp = SamplingParams(max_tokens=10, temperature=0.0, ignore_eos=True)
    gm = LlamaModel(mc, "cuda", init="empty").copy_from(cpu_model)
    bf16_bytes = gm.weight_bytes()
    names = _launches(monkeypatch)
    kw = {"kv_dtype": kv_dtype} if kv_dtype else {}

    def engine(graphs):
        return LLMEngine(EngineConfig(model=name, device="cuda", num_blocks=128, max_num_seqs=4, max_model_len=512,
                                      max_num_batched_tokens=512, use_graphs=graphs, enable_prefix_caching=False,
                                      expert_quant="fp8", **kw), model_cfg=mc, model=gm)
    eager_eng = engine(False)
    assert gm.expert_quant == "fp8" and gm.weight_quant is None and isinstance(gm.layers[0].experts_down, ops.Fp8ExpertWeight)
    assert gm.layers[0].qkv.dtype == torch.bfloat16 and gm.layers[0].router.dtype == torch.bfloat16
    E, Im, H = mc.num_experts, mc.moe_intermediate_size, mc.hidden_size
    assert bf16_bytes - gm.weight_bytes() == len(gm.layers) * (3 * E * Im * H - 4 * E * (2 * Im + H))
    eager = [r.output for r in eager_eng.generate(prompts, sp)]
    torch.cuda.synchronize()
    assert "moe_gemm_w8" in names and "moe_gemm" not in names
    rec_outs, records = moe_gpu._recorded_run(eager_eng, prompts, sp)
    # the fp32 CPU model with the GPU's exact codes and scales
    f32 = LlamaModel(mc, "cpu", torch.float32, seed=1).quantize_experts("fp8").copy_from(gm)
    assert torch.equal(f32.layers[1].experts_gate_up.q.view(torch.uint8), gm.layers[1].experts_gate_up.q.cpu().view(torch.uint8))
    assert _teacher_forced_ok(name, f32, prompts, rec_outs, records, kv_dtype=kv_dtype) == 30
    if kv_dtype is None:
        assert [r.output for r in eager_eng.generate(prompts, sp)] == eager          # run to run
        graph_eng = engine(True)
        graph = [r.output for r in graph_eng.generate(prompts, sp)]
        assert graph == eager
        assert [r.output for r in graph_eng.generate(prompts, sp)] == eager          # and again
