"""Qwen3-MoE on the GPU: the four MoE kernels (dgi/csrc/moe.hip) against their torch definitions,
``ops.moe_mlp`` eager and in a graph, and the engine on ``qwen3-moe-tiny`` and on a Hugging Face
``Qwen3MoeForCausalLM`` checkpoint (the CPU side: tests/test_moe.py)."""
import numpy as np
import pytest
import torch

from dgi import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
GEMM_ATOL, GEMM_RTOL = 3e-2, 2e-2      # the skinny GEMM's bound in tests/test_kernels_gpu.py


@pytest.fixture(autouse=True, scope="module")
def _native():
    ops.load_native(required=True)


def _launches(monkeypatch):
    names = []
    orig = ops._call

    def spy(name, *a):
        names.append(name)
        return orig(name, *a)
    monkeypatch.setattr(ops, "_call", spy)
    return names


# ---------------------------------------------------------------------------- moe_route

ROUTE_CASES = [(1, 8, 2), (5, 128, 8), (67, 64, 6), (33, 60, 4), (300, 256, 8)]


@pytest.mark.parametrize("T,E,k", ROUTE_CASES)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_moe_route(T, E, k, dtype, monkeypatch):
    g = torch.Generator().manual_seed(T * 1000 + E)
    # a permutation of 0.125 * arange(E) per row: distinct and exact in bf16
    rows = torch.stack([0.125 * torch.randperm(E, generator=g).float() for _ in range(T)])
    assert torch.equal(rows.to(dtype).float(), rows)
    names = _launches(monkeypatch)
    want = torch.topk(rows, k, dim=-1).indices
    l64 = rows.double()
    ex = torch.exp(l64 - l64.max(-1, keepdim=True).values)
    for norm in (True, False):
        ids, w = ops.moe_route(rows.to(dtype).to(DEV), k, norm)
        assert ids.dtype == torch.int32 and w.dtype == torch.float32 and ids.shape == w.shape == (T, k)
        assert torch.equal(ids.cpu().long(), want)
        p = ex.gather(-1, want)
        ref = p / (p.sum(-1, keepdim=True) if norm else ex.sum(-1, keepdim=True))
        torch.testing.assert_close(w.cpu().double(), ref, atol=2e-5, rtol=1e-5)
    assert names == ["moe_route", "moe_route"]
    # all-equal logits: ties go to the lower expert, equal weights
    flat = torch.full((T, E), 1.5, dtype=dtype, device=DEV)
    ids, w = ops.moe_route(flat, k, True)
    assert torch.equal(ids.cpu(), torch.arange(k, dtype=torch.int32).expand(T, k))
    assert torch.equal(w.cpu(), torch.full((T, k), 1.0 / k))
    _, w = ops.moe_route(flat, k, False)
    torch.testing.assert_close(w.cpu(), torch.full((T, k), 1.0 / E), atol=1e-7, rtol=1e-6)


def test_moe_route_matches_its_definition_on_ties_and_strided_rows():
    g = torch.Generator().manual_seed(3)
    wide = torch.randint(-3, 4, (41, 80), generator=g).float().mul(0.5).bfloat16().to(DEV)    # many ties
    logits = wide[:, :60]                                                                      # row stride 80
    for k in (1, 5, 16):
        ids, w = ops.moe_route(logits, k, True)
        rid, rw = ops.moe_route_ref(logits.cpu(), k, True)
        assert torch.equal(ids.cpu(), rid)
        torch.testing.assert_close(w.cpu(), rw, atol=2e-5, rtol=1e-5)


# ---------------------------------------------------------------------------- moe_align

def _align_py(ids, E, BM):
    """The layout in plain Python / numpy: expert by expert, slots in ascending order."""
    flat = np.asarray(ids).reshape(-1)
    n = flat.size
    P = BM * (-(-n // BM) + min(E, n))
    sorted_slot = np.full(P, -1, np.int32)
    block_expert = np.full(P // BM, -1, np.int32)
    inv = np.full(n, -1, np.int32)
    counts = np.zeros(E, np.int32)
    offsets = np.zeros(E + 1, np.int32)
    off = 0
    for e in range(E):
        slots = np.nonzero(flat == e)[0]
        counts[e] = slots.size
        offsets[e] = off
        sorted_slot[off:off + slots.size] = slots
        inv[slots] = off + np.arange(slots.size)
        pad = -(-slots.size // BM) * BM
        block_expert[off // BM:(off + pad) // BM] = e
        off += pad
    offsets[E] = off
    return counts, offsets, sorted_slot, block_expert, inv


def _align_inputs():
    g = torch.Generator().manual_seed(0)
    yield "random", torch.randint(0, 60, (37, 4), generator=g, dtype=torch.int32), 60
    yield "one expert", torch.full((50, 2), 3, dtype=torch.int32), 8
    yield "fewer slots than experts", torch.tensor([[5, 90, 17]], dtype=torch.int32), 128
    yield "8192 x 8", torch.randint(0, 128, (8192, 8), generator=g, dtype=torch.int32), 128


@pytest.mark.parametrize("BM", [16, 32])
def test_moe_align(BM, monkeypatch):
    names = _launches(monkeypatch)
    for what, ids, E in _align_inputs():
        n = ids.numel()
        ref = _align_py(ids.numpy(), E, BM)
        got = [t.cpu().numpy() for t in ops.moe_align(ids.to(DEV), E, BM)]
        again = [t.cpu().numpy() for t in ops.moe_align(ids.to(DEV), E, BM)]
        for name, r, a, b in zip(("counts", "offsets", "sorted_slot", "block_expert", "inv"), ref, got, again):
            assert a.dtype == np.int32 and np.array_equal(a, r), (what, name)
            assert np.array_equal(a, b), (what, name, "second run")
        counts, offsets, sorted_slot, block_expert, inv = got
        assert sorted_slot.size == ops.moe_capacity(n, E, BM) and block_expert.size == sorted_slot.size // BM
        real = sorted_slot[sorted_slot >= 0]
        assert np.array_equal(np.sort(real), np.arange(n)), what                # every slot exactly once
        assert np.array_equal(sorted_slot[inv], np.arange(n)), what              # inv inverts sorted_slot
        flat = ids.numpy().reshape(-1)
        for e in range(E):
            seg = sorted_slot[offsets[e]:offsets[e + 1]]
            assert np.all(seg[:counts[e]] >= 0) and np.all(np.diff(seg[:counts[e]]) > 0), (what, e)   # ascending
            assert np.all(flat[seg[:counts[e]]] == e) and np.all(seg[counts[e]:] == -1), (what, e)    # padding
            assert np.all(block_expert[offsets[e] // BM:offsets[e + 1] // BM] == e), (what, e)
        assert np.all(sorted_slot[offsets[E]:] == -1) and np.all(block_expert[offsets[E] // BM:] == -1), what
    assert names and set(names) == {"moe_align"}


# ---------------------------------------------------------------------------- moe_gemm

def _nan_like(*shape):
    return torch.full(shape, float("nan"), dtype=torch.bfloat16, device=DEV)


def _exact_case(counts, K, N, BM, seed):
    """Plain epilogue on {-1, 0, 1} operands: fp32 accumulation is exact, so every real row must equal
    bf16(x @ w[e]^T) bit for bit; x's padding rows and the output start as NaN."""
    g = torch.Generator().manual_seed(seed)
    E = len(counts)
    ids = torch.cat([torch.full((c,), e, dtype=torch.int32) for e, c in enumerate(counts)])
    ids = ids[torch.randperm(ids.numel(), generator=g)].reshape(-1, 1)          # k = 1: slot = token
    _c, _o, sorted_slot, block_expert, inv = ops.moe_align(ids.to(DEV), E, BM)
    P = sorted_slot.numel()
    w = torch.randint(-1, 2, (E, N, K), generator=g).bfloat16()
    xt = torch.randint(-1, 2, (ids.numel(), K), generator=g).bfloat16()        # per token
    xs = _nan_like(P, K)
    xs[inv.long()] = xt.to(DEV)
    out = _nan_like(P, N)
    ops.moe_gemm(xs, w.to(DEV), sorted_slot, block_expert, 1, ops.MOE_EPI_PLAIN, BM, out=out)
    out = out.cpu()
    slot = sorted_slot.cpu().long()
    real = slot >= 0
    assert torch.isfinite(out[real].float()).all() and torch.isnan(out[~real].float()).all()
    ref = torch.stack([(xt[t].float() @ w[int(ids[t, 0])].float().t()) for t in range(ids.numel())]).bfloat16()
    assert torch.equal(out[inv.cpu().long()], ref)


@pytest.mark.parametrize("BM", [16, 32])
@pytest.mark.parametrize("K,N", [(256, 512), (768, 2048), (768, 512), (256, 2048)])
def test_moe_gemm_exact(K, N, BM, monkeypatch):
    names = _launches(monkeypatch)
    _exact_case([0, 1, 15, 16, 17, 33], K, N, BM, seed=K + N)
    _exact_case([0, 0, 40, 0], K, N, BM, seed=K + N + 1)                       # every row in one expert
    assert names.count("moe_gemm") == 2


def _random_layout(T, k, E, BM, g):
    ids = torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(T)]).to(torch.int32)
    return ids, ops.moe_align(ids.to(DEV), E, BM)


@pytest.mark.parametrize("T,k,E,K,N,BM", [(7, 4, 8, 2048, 768, 16), (45, 2, 5, 2048, 768, 32), (33, 3, 6, 512, 272, 16)])
def test_moe_gemm_swiglu_random(T, k, E, K, N, BM, monkeypatch):
    """SwiGLU epilogue over [gate; up] [E, 2N, K], rows gathered through sorted_slot // k.  Every
    token's row is distinct at O(1), so a wrong gather row lands far outside the bound."""
    g = torch.Generator().manual_seed(T + K)
    names = _launches(monkeypatch)
    ids, (_c, _o, sorted_slot, block_expert, inv) = _random_layout(T, k, E, BM, g)
    x = torch.randn(T, K, generator=g).bfloat16()
    w = (torch.randn(E, 2 * N, K, generator=g) / K ** 0.5).bfloat16()
    out = _nan_like(sorted_slot.numel(), N)
    ops.moe_gemm(x.to(DEV), w.to(DEV), sorted_slot, block_expert, k, ops.MOE_EPI_SWIGLU, BM, out=out)
    assert names.count("moe_gemm") == 1
    ref = ops.moe_gemm_ref(x, w, sorted_slot.cpu(), block_expert.cpu(), k, ops.MOE_EPI_SWIGLU, BM,
                           out=torch.full((sorted_slot.numel(), N), float("nan"), dtype=torch.bfloat16))
    out = out.cpu()
    real = sorted_slot.cpu() >= 0
    assert int(real.sum()) == T * k and torch.isnan(out[~real].float()).all() and torch.isnan(ref[~real].float()).all()
    assert float(ref[real].float().abs().max()) > 0.5
    torch.testing.assert_close(out[real].float(), ref[real].float(), atol=GEMM_ATOL, rtol=GEMM_RTOL)


@pytest.mark.parametrize("T,k,E,K,N,BM", [(9, 4, 8, 768, 2048, 16), (50, 2, 5, 768, 2048, 32)])
def test_moe_gemm_plain_random(T, k, E, K, N, BM):
    g = torch.Generator().manual_seed(T + K)
    ids, (_c, _o, sorted_slot, block_expert, inv) = _random_layout(T, k, E, BM, g)
    P = sorted_slot.numel()
    xs = torch.randn(P, K, generator=g).bfloat16()
    w = (torch.randn(E, N, K, generator=g) / K ** 0.5).bfloat16()
    out = ops.moe_gemm(xs.to(DEV), w.to(DEV), sorted_slot, block_expert, k, ops.MOE_EPI_PLAIN, BM).cpu()
    ref = ops.moe_gemm_ref(xs, w, sorted_slot.cpu(), block_expert.cpu(), k, ops.MOE_EPI_PLAIN, BM)
    real = sorted_slot.cpu() >= 0
    torch.testing.assert_close(out[real].float(), ref[real].float(), atol=GEMM_ATOL, rtol=GEMM_RTOL)


# ---------------------------------------------------------------------------- moe_combine

@pytest.mark.parametrize("T,k,E,H", [(19, 4, 8, 512), (3, 8, 128, 2048), (70, 2, 5, 520)])
def test_moe_combine_exact(T, k, E, H, monkeypatch):
    """Power-of-two weights and small-integer y: every product and sum is exact.  Padding rows of y
    are NaN and must never reach the output."""
    g = torch.Generator().manual_seed(T)
    names = _launches(monkeypatch)
    ids, (_c, _o, sorted_slot, _b, inv) = _random_layout(T, k, E, 16, g)
    P = sorted_slot.numel()
    # multiples of 1/4 up to 2 * k <= 16: exact in fp32 and in bf16's 8 significant bits
    y = torch.randint(-2, 3, (P, H), generator=g).bfloat16()
    y[sorted_slot.cpu() < 0] = float("nan")
    w = torch.pow(2.0, -torch.randint(0, 3, (T, k), generator=g).float())
    out = ops.moe_combine(y.to(DEV), inv, w.to(DEV)).cpu()
    assert names.count("moe_combine") == 1
    ref = torch.zeros(T, H, dtype=torch.float64)
    for j in range(k):
        ref += w[:, j, None].double() * y[inv.cpu().view(T, k)[:, j].long()].double()
    assert torch.isfinite(out.float()).all()
    assert torch.equal(out, ref.bfloat16()) and torch.equal(out.double(), ref)
    assert torch.equal(out, ops.moe_combine_ref(y, inv.cpu(), w))


# ---------------------------------------------------------------------------- moe_mlp

def _mlp_weights(E, H, I, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=DEV)       # noqa: E731
    # router logits of O(1): a bf16 ulp of a logit moves a routing weight by well under a percent
    return ((rn(E, H) / H ** 0.5).bfloat16(), (rn(E, 2 * I, H) / H ** 0.5).bfloat16(), (rn(E, H, I) / I ** 0.5).bfloat16(),
            lambda T: rn(T, H).bfloat16())


@pytest.mark.parametrize("E,k,H,I,Ts", [(8, 2, 512, 256, (1, 17, 300)), (128, 8, 2048, 768, (1, 40))])
def test_moe_mlp(E, k, H, I, Ts, monkeypatch):
    router, gate_up, down, make_x = _mlp_weights(E, H, I, seed=E)
    names = _launches(monkeypatch)
    # as the engine does: its captures run in inference mode, and so does every capture after one of them
    with torch.inference_mode():
        for T in Ts:
            x = make_x(T)
            names.clear()
            out = ops.moe_mlp(x, router, gate_up, down, k, True)
            assert [n for n in names if n.startswith("moe_")] == ["moe_route", "moe_align", "moe_gemm", "moe_gemm",
                                                                   "moe_combine"]
            assert torch.equal(out, ops.moe_mlp(x, router, gate_up, down, k, True)), T         # bit-reproducible
            ids, _ = ops.moe_route(ops.linear(x, router), k, True)
            forced = ops.moe_mlp(x, router, gate_up, down, k, True, ids=ids)
            ref = ops.moe_mlp_ref(x, router, gate_up, down, k, True, ids=ids)                  # the per-expert torch loop
            assert float(ref.float().abs().max()) > 0.05
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


def test_refusals_take_the_reference_and_never_launch(monkeypatch):
    g = torch.Generator().manual_seed(0)
    names = _launches(monkeypatch)
    # K % 256 != 0
    ids, (_c, _o, sorted_slot, block_expert, inv) = _random_layout(6, 2, 4, 16, g)
    x = torch.randn(6, 320, generator=g).bfloat16().to(DEV)
    w = (torch.randn(4, 64, 320, generator=g) / 16).bfloat16().to(DEV)
    names.clear()
    out = ops.moe_gemm(x, w, sorted_slot, block_expert, 2, ops.MOE_EPI_SWIGLU, 16)
    assert "moe_gemm" not in names
    assert torch.equal(out, ops.moe_gemm_ref(x, w, sorted_slot, block_expert, 2, ops.MOE_EPI_SWIGLU, 16))
    with pytest.raises(RuntimeError):
        torch.ops.dgi.moe_gemm(torch.empty(sorted_slot.numel(), 32, dtype=torch.bfloat16, device=DEV), x, w,
                               sorted_slot, block_expert, 2, 12, 1, 16)
    # E > 256 and k > 16
    for E, k in ((300, 4), (64, 17)):
        logits = torch.randn(5, E, generator=g).to(DEV)
        names.clear()
        ids, wts = ops.moe_route(logits, k, True)
        assert names == []
        rid, rw = ops.moe_route_ref(logits, k, True)
        assert torch.equal(ids, rid) and torch.equal(wts, rw)
        with pytest.raises(RuntimeError):
            torch.ops.dgi.moe_route(torch.empty(5, k, dtype=torch.int32, device=DEV),
                                    torch.empty(5, k, dtype=torch.float32, device=DEV), logits, k, True)
    names.clear()
    big = torch.randint(0, 300, (9, 2), generator=g, dtype=torch.int32).to(DEV)
    got = ops.moe_align(big, 300, 16)
    assert names == [] and all(torch.equal(a, b) for a, b in zip(got, ops.moe_align_ref(big, 300, 16)))
    # a whole block the kernels refuse is the reference
    router, gate_up, down, make_x = _mlp_weights(4, 320, 256, seed=1)
    xx = make_x(3)
    names.clear()
    out = ops.moe_mlp(xx, router, gate_up, down, 2, True)
    assert not [n for n in names if n.startswith("moe_")]
    assert torch.equal(out, ops.moe_mlp_ref(xx, router, gate_up, down, 2, True))


# ---------------------------------------------------------------------------- model: Hugging Face parity

H, IM, L, NH, NKV, HD, V, E, K = 512, 256, 2, 8, 2, 128, 1024, 8, 2       # qwen3-moe-tiny's geometry
HF_PROMPTS = [[1, 33, 44, 55, 66, 77, 88, 99, 111, 222], [1] + list(range(300, 300 + 139))]     # 10 and 140 tokens


def _tol(ref):
    return 0.03 * float(ref.abs().max()) + 0.02


def _hf_moe_model(seed):
    transformers = pytest.importorskip("transformers")
    cfg = transformers.Qwen3MoeConfig(vocab_size=V, hidden_size=H, intermediate_size=1024, moe_intermediate_size=IM,
                                      num_hidden_layers=L, num_attention_heads=NH, num_key_value_heads=NKV,
                                      head_dim=HD, num_experts=E, num_experts_per_tok=K, norm_topk_prob=True,
                                      decoder_sparse_step=1, mlp_only_layers=[], max_position_embeddings=1024,
                                      rms_norm_eps=1e-6, bos_token_id=1, eos_token_id=2, tie_word_embeddings=False,
                                      rope_theta=1000000.0)
    model = transformers.Qwen3MoeForCausalLM(cfg)
    torch.manual_seed(seed)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "norm" in n:
                p.copy_(1.0 + 0.1 * torch.randn_like(p))
            else:
                p.normal_(0.0, 0.04)
    return model.eval().float()


def _force_hf_routing(model, record, seen):
    """Patch every router of the HF model: rows with a recorded (layer, position) use those experts,
    with HF's own probabilities at them; ``seen[layer]`` keeps the router logits."""
    for li, layer in enumerate(model.model.layers):
        gate = layer.mlp.gate

        def forward(hidden_states, _g=gate, _li=li):
            logits = torch.nn.functional.linear(hidden_states.reshape(-1, _g.hidden_dim), _g.weight)
            probs = torch.softmax(logits, dim=-1, dtype=torch.float)
            idx = torch.topk(probs, _g.top_k, dim=-1).indices
            for r in range(idx.shape[0]):
                if (_li, r) in record:
                    idx[r] = torch.tensor(record[(_li, r)])
            top = probs.gather(-1, idx)
            top = top / top.sum(-1, keepdim=True)            # norm_topk_prob
            seen[_li] = logits.detach()
            return logits, top.to(logits.dtype), idx
        gate.forward = forward


def test_gpu_bf16_per_step_logits_match_hf_with_the_routing_held_fixed(tmp_path):
    """The dense Qwen3 test (tests/test_qwen3_gpu.py) with the one discontinuity taken out: HF fp32
    runs on prompt + GPU tokens with its routers forced to the experts the GPU chose, and every step's
    GPU logits are held to 0.03 * max|ref| + 0.02, cosine > 0.999, chosen token within the bound of
    the maximum.  Separately, every expert the GPU chose must be legitimate: within
    2 * (0.03 * max|l| + 0.02) of the k-th largest of the forced fp32 run's router logits l."""
    from dgi.engine import EngineConfig, LLMEngine
    from dgi.sched.request import SamplingParams
    model = _hf_moe_model(0)
    model.save_pretrained(str(tmp_path), safe_serialization=True)
    eng = LLMEngine(EngineConfig(model_path=str(tmp_path), device="cuda", dtype=torch.bfloat16, num_blocks=128,
                                 max_num_seqs=4, max_model_len=512, max_num_batched_tokens=256, use_graphs=False,
                                 enable_prefix_caching=False))
    assert eng.model.cfg.arch == "qwen3_moe" and eng.model.layers[0].experts_gate_up.is_cuda
    sd = model.state_dict()
    assert torch.equal(eng.model.layers[1].experts_down.cpu(), sd["model.layers.1.mlp.experts.down_proj"].bfloat16())
    steps, record = [], {}
    orig = eng.model.compute_logits

    def spy(h, residual, idx):
        out = orig(h, residual, idx)
        steps.append(out.detach().float().cpu())
        return out

    def hook(layer, positions, ids, weights):
        for p, row in zip(positions.tolist(), ids.tolist()):
            record[(layer, p)] = row
        return None
    eng.model.compute_logits = spy
    eng.model.route_hook = hook
    n_new = 12
    sp = SamplingParams(max_tokens=n_new, temperature=0.0, ignore_eos=True)
    worst = worst_route = 0.0
    for prompt in HF_PROMPTS:
        steps.clear()
        record.clear()
        toks = eng.generate([prompt], sp)[0].output
        assert len(toks) == n_new and len(steps) == n_new
        n = len(prompt) + n_new
        assert all((0, p) in record for p in range(n - 1))
        assert all((L - 1, len(prompt) - 1 + t) in record for t in range(n_new))
        seen = {}
        _force_hf_routing(model, record, seen)
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
        for (layer, p), chosen in record.items():
            row = seen[layer][p]
            kth = float(row.topk(K).values[-1])
            allow = 2.0 * (0.03 * float(row.abs().max()) + 0.02)
            for e in chosen:
                ratio = (kth - float(row[e])) / allow
                worst_route = max(worst_route, ratio)
                assert ratio <= 1.0, (layer, p, e, float(row[e]), kth, allow)
    print(f"worst logit error / bound: {worst:.3f}; worst routing shortfall / allowance: {worst_route:.3f}")


# ---------------------------------------------------------------------------- model: engine

def _count_mlp(monkeypatch):
    calls = []
    orig = ops.moe_mlp

    def counted(x, *a, **k):
        calls.append(x.shape[0])
        return orig(x, *a, **k)
    monkeypatch.setattr(ops, "moe_mlp", counted)
    return calls


def _teacher_forced_ok(name, src_model, prompts, gpu_outs, records, rel=0.03, abs_=0.02, kv_dtype=None):
    """tests/test_qwen3_gpu._teacher_forced_ok with the routing held fixed: every token the GPU chose
    is an argmax of the fp32 CPU model's logits for the same prefix (teacher forced) up to a bf16
    tolerance, where the CPU model's routers use the experts the GPU recorded per (layer, position)."""
    from dgi.engine import EngineConfig, LLMEngine
    from dgi.models.llama import LlamaModel
    from dgi.sched.request import SamplingParams
    mc = src_model.cfg
    f32 = LlamaModel(mc, "cpu", torch.float32, init="empty").copy_from(src_model)
    kw = {"kv_dtype": kv_dtype} if kv_dtype else {}
    ref = LLMEngine(EngineConfig(model=name, device="cpu", dtype=torch.float32, num_blocks=256, max_num_seqs=8,
                                 max_model_len=512, max_num_batched_tokens=512, use_graphs=False,
                                 enable_prefix_caching=False, **kw), model_cfg=mc, model=f32)
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
    for p, toks, rec in zip(prompts, gpu_outs, records):
        cur["rec"] = rec
        for t, tok in enumerate(toks):
            ref.generate([p + toks[:t]], one)
            r = got["l"]
            tol = rel * float(r.abs().max()) + abs_
            worst = max(worst, (float(r.max()) - float(r[tok])) / tol)
            assert float(r[tok]) >= float(r.max()) - tol, (name, len(p), t, tok, int(r.argmax()))
            checked += 1
    print(f"{name} kv={kv_dtype}: {checked} tokens, worst (max - chosen) / tol = {worst:.3f}")
    return checked


def _recorded_run(eng, prompts, sp):
    """Each prompt alone through an eager engine, its routing recorded per (layer, position)."""
    outs, records = [], []
    for p in prompts:
        rec = {}

        def hook(layer, positions, ids, weights, _rec=rec):
            for pos, row in zip(positions.tolist(), ids.tolist()):
                _rec[(layer, pos)] = row
            return None
        eng.model.route_hook = hook
        outs.append(eng.generate([p], sp)[0].output)
        records.append(rec)
    eng.model.route_hook = None
    return outs, records


@pytest.mark.parametrize("kv_dtype", [None, "fp8"])
def test_moe_engine_gpu(kv_dtype, monkeypatch):
    """qwen3-moe-tiny through the native kernels: graphs == eager, run to run, and every token is
    within the bound of the fp32 CPU engine's maximum with the routing the GPU recorded."""
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
    calls = _count_mlp(monkeypatch)
    kw = {"kv_dtype": kv_dtype} if kv_dtype else {}

    def engine(graphs):
        return LLMEngine(EngineConfig(model=name, device="cuda", num_blocks=128, max_num_seqs=4, max_model_len=512,
                                      max_num_batched_tokens=512, use_graphs=graphs, enable_prefix_caching=False, **kw),
                         model_cfg=mc, model=gm)
    eager_eng = engine(False)
    assert eager_eng.mlp_pad_table is None and gm.mlp_impl is None and not gm.norms_folded
    eager = [r.output for r in eager_eng.generate(prompts, sp)]
    torch.cuda.synchronize()
    assert max(calls) >= 300 and min(calls) <= 3
    rec_outs, records = _recorded_run(eager_eng, prompts, sp)
    assert _teacher_forced_ok(name, cpu_model, prompts, rec_outs, records, kv_dtype=kv_dtype) == 30
    if kv_dtype is None:
        assert [r.output for r in eager_eng.generate(prompts, sp)] == eager          # run to run
        graph_eng = engine(True)
        graph = [r.output for r in graph_eng.generate(prompts, sp)]
        assert graph == eager
        assert [r.output for r in graph_eng.generate(prompts, sp)] == eager          # and again
        gm.route_hook = lambda *a: None
        monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="route_hook"):                         # never inside a capture
            gm._mlp(0, gm.layers[0], torch.zeros(2, mc.hidden_size, dtype=torch.bfloat16, device=DEV),
                    torch.zeros(2, dtype=torch.int32, device=DEV))
        gm.route_hook = None
