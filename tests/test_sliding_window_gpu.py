"""Sliding-window paged_decode / paged_prefill on an MI355X (``pytest -m gpu``): inputs whose answer
is known exactly (tests/swa_cases.py) through every launch plan, block size, tile configuration and
KV format, with every K/V slot the read contract forbids poisoned; no-window calls bit-equal to the
call without the argument; a captured decode launch replayed across the window edge; the engine on
the two windowed tiny models; the binding's refusals.  Each test prints its worst error / tolerance
ratio (``RATIO ...`` lines, ``pytest -s``).
"""
import pytest
import torch

import attn_cases as ac
import swa_cases as sw
from dgi import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"

DECODE_SHAPES = [(32, 8, 128), (14, 2, 64)]
WINDOWS = [1, 16, 31, 32, 33, 64, 100, 128, 1000]
PREFILL_SHAPES = [(32, 8, 128), (14, 2, 64)]
PREFILL_PAIRS = [([65], [65]), ([257], [1000]), ([129, 0, 33], [129, 50, 600]), ([128], [191])]
PREFILL_WINDOWS = [1, 33, 64, 100, 200]
PREFILL_CFGS = [(128, 1), (128, 0), (256, 1), (256, 0)]            # (PREFILL_TILE, PREFILL_DB)
BLOCK_SIZES = [8, 16, 32, 64]
KV = ["bf16", "fp8"]


def decode_ctxs(W):
    return sorted({c for c in (1, W - 1, W, W + 1, W + 31, W + 32, W + 33, 2 * W + 5, 2049) if c >= 1})


@pytest.fixture(autouse=True, scope="module")
def _native():
    ops.load_native(required=True)


def _report(failures, worst, what):
    print(f"RATIO swa {what} {worst:.4f}")
    assert not failures, "\n".join(failures)


def _decode_plans(w):
    """(plan name, output) for every launch plan the unwindowed exact tests drive, with the window."""
    c = w.c
    B, nh, nkv, hd = len(c.ctxs), c.nh, c.nkv, c.hd
    args = (c.q, w.kc, w.vc, c.bt, c.ctx, nh, nkv, c.scale)
    kw = dict(kv_scale=w.kv_scale, window=w.window)
    mx = max(c.ctxs)
    yield "one split", ops.paged_decode(*args, 1, 1 << 20, **kw)
    splits, part = ops.decode_split_plan(B, mx, nkv)
    yield f"split plan {splits}x{part}", ops.paged_decode(*args, splits, part, **kw)
    yield "part 128, spare splits", ops.paged_decode(*args, (mx + 127) // 128 + 3, 128, **kw)
    ws2 = (torch.empty(B * nh * splits * hd, device=DEV), torch.empty(B * nh * splits, device=DEV))
    yield "reduce kernel", ops.paged_decode(*args, splits, part, workspace=ws2, **kw)
    for S, mn in ac.DEVICE_PLANS:
        ws = (torch.empty(B * nh * S * hd, device=DEV), torch.empty(B * nh * S, device=DEV),
              torch.zeros(B * nkv, dtype=torch.int32, device=DEV))
        for rep in range(2):
            yield f"device plan S={S} min={mn} run {rep}", ops.paged_decode(*args, S, -mn, workspace=ws, **kw)
        assert int(ws[2].abs().sum()) == 0, f"ticket counters not back to zero (S={S}, min={mn})"


def _decode_case(family, nh, nkv, hd, ctxs, W, kv, bs=16, plans=_decode_plans):
    w = sw.build(family, nh, nkv, hd, ctxs, W, bs=bs, device=DEV, fp8=kv == "fp8")
    failures, worst = [], 0.0
    for name, out in plans(w):
        r = sw.check(w, out)
        worst = max(worst, r.ratio)
        if not r.ok:
            failures.append(f"W {W} {kv} {name}: {r.detail}")
    return failures, worst


@pytest.mark.parametrize("kv", KV)
@pytest.mark.parametrize("family", sw.FAMILIES)
@pytest.mark.parametrize("W", WINDOWS)
@pytest.mark.parametrize("nh,nkv,hd", DECODE_SHAPES)
def test_decode(nh, nkv, hd, W, family, kv):
    _report(*_decode_case(family, nh, nkv, hd, decode_ctxs(W), W, kv), f"{family} decode")


@pytest.mark.parametrize("kv", KV)
@pytest.mark.parametrize("family", sw.FAMILIES)
@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_decode_block_sizes(bs, family, kv):
    failures, worst = [], 0.0
    for W in (33, 100):
        f, r = _decode_case(family, 32, 8, 128, decode_ctxs(W), W, kv, bs=bs)
        failures += f
        worst = max(worst, r)
    _report(failures, worst, f"{family} decode bs={bs}")


@pytest.mark.parametrize("kv", KV)
@pytest.mark.parametrize("family", sw.FAMILIES)
def test_decode_40_sequences(family, kv):
    """B * nkv > 128: one split runs the 4-wave kernel."""
    def plans(w):
        c = w.c
        args = (c.q, w.kc, w.vc, c.bt, c.ctx, c.nh, c.nkv, c.scale)
        kw = dict(kv_scale=w.kv_scale, window=w.window)
        yield "one split (4 waves)", ops.paged_decode(*args, 1, 1 << 20, **kw)
        yield "part 128", ops.paged_decode(*args, (max(c.ctxs) + 127) // 128, 128, **kw)
    failures, worst = [], 0.0
    for W in (1, 33, 64, 100):
        ctxs = [c for c in decode_ctxs(W) if c != 2049]
        ctxs = (ctxs * 8)[:39] + [777]
        assert len(ctxs) == 40
        f, r = _decode_case(family, 32, 8, 128, ctxs, W, kv, plans=plans)
        failures += f
        worst = max(worst, r)
    _report(failures, worst, f"{family} decode 40 sequences")


def _prefill_case(monkeypatch, family, nh, nkv, hd, W, kv, bs=16, pairs=PREFILL_PAIRS):
    failures, worst = [], 0.0
    for qlens, ctxs in pairs:
        w = sw.build(family, nh, nkv, hd, ctxs, W, qlens, bs=bs, device=DEV, fp8=kv == "fp8")
        c = w.c
        for tile, db in PREFILL_CFGS:
            monkeypatch.setattr(ops, "PREFILL_TILE", tile)
            monkeypatch.setattr(ops, "PREFILL_DB", db)
            out = ops.paged_prefill(c.q, w.kc, w.vc, c.bt, c.cu, c.ctx, nh, nkv, c.scale, kv_scale=w.kv_scale,
                                    window=W)
            r = sw.check(w, out)
            worst = max(worst, r.ratio)
            if not r.ok:
                failures.append(f"W {W} {kv} qlens {qlens} ctxs {ctxs} tile {tile} db {db}: {r.detail}")
    return failures, worst


@pytest.mark.parametrize("kv", KV)
@pytest.mark.parametrize("family", sw.FAMILIES)
@pytest.mark.parametrize("W", PREFILL_WINDOWS)
@pytest.mark.parametrize("nh,nkv,hd", PREFILL_SHAPES)
def test_prefill(nh, nkv, hd, W, family, kv, monkeypatch):
    """([257], [1000]) with W = 33 (and W = 1, 64, 100 under 256-row tiles) has rows whose leading
    K/V tiles hold none of their keys: they must contribute exactly nothing."""
    _report(*_prefill_case(monkeypatch, family, nh, nkv, hd, W, kv), f"{family} prefill")


@pytest.mark.parametrize("family", sw.FAMILIES)
@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_prefill_block_sizes(bs, family, monkeypatch):
    _report(*_prefill_case(monkeypatch, family, 32, 8, 128, 33, "bf16", bs=bs,
                           pairs=[([257], [1000]), ([129, 0, 33], [129, 50, 600])]), f"{family} prefill bs={bs}")


# ---------------------------------------------------------------------------- no window

@pytest.mark.parametrize("kv", KV)
def test_no_window_is_bit_equal(kv, monkeypatch):
    """window = 0 and W >= ctx against the call without the argument, under the same plan."""
    ctxs = [1, 33, 129, 700]
    c = ac.build("D", 32, 8, 128, ctxs, device=DEV)
    sc, kc, vc = None, c.kc, c.vc
    if kv == "fp8":
        sc = torch.ones(2, 8, device=DEV)
        kc = ops.quantize_kv_ref(c.kc.transpose(1, 2), sc[0]).transpose(1, 2).contiguous()
        vc = ops.quantize_kv_ref(c.vc.transpose(1, 2), sc[1]).transpose(1, 2).contiguous()
    args = (c.q, kc, vc, c.bt, c.ctx, 32, 8, c.scale)
    B, nh, hd = len(ctxs), 32, 128
    splits, part = ops.decode_split_plan(B, max(ctxs), 8)

    def ws(S, counters):
        t = (torch.empty(B * nh * S * hd, device=DEV), torch.empty(B * nh * S, device=DEV))
        return t + ((torch.zeros(B * 8, dtype=torch.int32, device=DEV),) if counters else ())
    plans = [dict(max_splits=1, part_size=1 << 20), dict(max_splits=splits, part_size=part),
             dict(max_splits=splits, part_size=part, workspace=ws(splits, False)),
             dict(max_splits=16, part_size=-64, workspace=ws(16, True)),
             dict(max_splits=3, part_size=-32, workspace=ws(3, True))]
    for plan in plans:
        base = ops.paged_decode(*args, kv_scale=sc, **plan)
        assert not bool(torch.isnan(base).any())
        for W in (0, 700, 701, 1 << 20):
            assert torch.equal(ops.paged_decode(*args, kv_scale=sc, window=W, **plan), base), (plan, W)
    qlens = [1, 33, 129, 300]
    p = ac.build("D", 32, 8, 128, ctxs, qlens, device=DEV)
    kc, vc = p.kc, p.vc
    if kv == "fp8":
        kc = ops.quantize_kv_ref(p.kc.transpose(1, 2), sc[0]).transpose(1, 2).contiguous()
        vc = ops.quantize_kv_ref(p.vc.transpose(1, 2), sc[1]).transpose(1, 2).contiguous()
    for tile, db in PREFILL_CFGS:
        monkeypatch.setattr(ops, "PREFILL_TILE", tile)
        monkeypatch.setattr(ops, "PREFILL_DB", db)
        base = ops.paged_prefill(p.q, kc, vc, p.bt, p.cu, p.ctx, 32, 8, p.scale, kv_scale=sc)
        assert not bool(torch.isnan(base).any())
        for W in (0, 700, 701, 1 << 20):
            got = ops.paged_prefill(p.q, kc, vc, p.bt, p.cu, p.ctx, 32, 8, p.scale, kv_scale=sc, window=W)
            assert torch.equal(got, base), (tile, db, W)


# ---------------------------------------------------------------------------- graph

def test_captured_decode_follows_the_context_across_the_window_edge():
    """One captured launch with the device-side plan, replayed while context_lens grows in place
    from W - 2 to W + 40: the window start, the plan's base and the split count all move."""
    # as the engine does: its captures run in inference mode, and so does every capture after one of them
    with torch.inference_mode():
        _captured_decode_body()


def _captured_decode_body():
    W, nh, nkv, hd, B, S = 64, 32, 8, 128, 3, 16
    top = W + 40 + 70
    c = ac.build("D", nh, nkv, hd, [top] * B, device=DEV)
    # finite K/V everywhere the sequences can reach (the pool's slots past `top` stay NaN)
    ctx = torch.zeros(B, dtype=torch.int32, device=DEV)
    out = torch.empty(B, nh * hd, dtype=torch.bfloat16, device=DEV)
    ws = (torch.empty(B * nh * S * hd, device=DEV), torch.empty(B * nh * S, device=DEV),
          torch.zeros(B * nkv, dtype=torch.int32, device=DEV))
    offs = torch.tensor([0, 33, 70], dtype=torch.int32, device=DEV)

    def launch(o):
        return ops.paged_decode(c.q, c.kc, c.vc, c.bt, ctx, nh, nkv, c.scale, S, -32, out=o, workspace=ws, window=W)
    ctx.copy_(offs + W - 2)
    launch(out)                                   # warm up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch(out)
    eager = torch.empty_like(out)
    for n in range(W - 2, W + 41):
        ctx.copy_(offs + n)
        g.replay()
        launch(eager)
        torch.cuda.synchronize()
        assert torch.equal(out, eager) and not bool(torch.isnan(out).any()), n
    assert int(ws[2].abs().sum()) == 0


# ---------------------------------------------------------------------------- engine

def _engine(name, mc, model, graphs, kv_dtype=None):
    from dgi.engine import EngineConfig, LLMEngine
    kw = {"kv_dtype": kv_dtype} if kv_dtype else {}
    return LLMEngine(EngineConfig(model=name, device="cuda", num_blocks=256, max_num_seqs=8, max_model_len=512,
                                  max_num_batched_tokens=64, use_graphs=graphs, **kw), model_cfg=mc, model=model)


def _teacher_forced_ok(name, src_model, prompts, gpu_outs, kv_dtype, rel=0.03, abs_=0.02):
    """The engine tests' check (test_kernels_gpu / test_kv_fp8_gpu), same tolerance: every token the GPU
    chose is an argmax of the fp32 CPU model's logits for the same prefix, up to a bf16 tolerance;
    with an fp8 KV cache the reference engine runs on an fp8 pool too."""
    from dgi.engine import EngineConfig, LLMEngine
    from dgi.models.llama import LlamaModel
    from dgi.sched.request import SamplingParams
    mc = src_model.cfg
    f32 = LlamaModel(mc, "cpu", torch.float32, init="empty").copy_from(src_model)
    kw = {"kv_dtype": kv_dtype} if kv_dtype else {}
    ref = LLMEngine(EngineConfig(model=name, device="cpu", dtype=torch.float32, num_blocks=256, max_num_seqs=8,
                                 max_model_len=512, max_num_batched_tokens=256, use_graphs=False,
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
    for p, toks in zip(prompts, gpu_outs):
        for t, tok in enumerate(toks):
            ref.generate([p + toks[:t]], one)
            r = got["l"]
            tol = rel * float(r.abs().max()) + abs_
            assert float(r[tok]) >= float(r.max()) - tol, (name, len(p), t, tok, int(r.argmax()))
            checked += 1
    return checked


@pytest.mark.parametrize("kv_dtype", [None, "fp8"])
@pytest.mark.parametrize("name", ["mistral-tiny", "qwen-tiny-swa"])
def test_engine_windowed_models(name, kv_dtype, monkeypatch):
    """100-token prompts (2.5 windows) in mixed steps — a 64-token budget, so decode rows run beside
    prefill chunks: graphs == eager, run to run, and every GPU token is teacher-forced against the
    fp32 CPU model."""
    from dgi.models.config import get_config
    from dgi.models.llama import LlamaModel
    from dgi.sched.request import SamplingParams
    mc = get_config(name)
    cpu_model = LlamaModel(mc, "cpu", seed=5)
    g = torch.Generator().manual_seed(11)
    prompts = [[1] + torch.randint(3, 1000, (n - 1,), generator=g).tolist() for n in (100, 37, 100)]
    sp = SamplingParams(max_tokens=8, temperature=0.0, ignore_eos=True)
    windows = {"paged_decode": set(), "paged_prefill": set()}
    mixed = [0]
    orig_call = ops._call

    def call(op, *args):
        if op in windows:
            windows[op].add(args[-1])
        return orig_call(op, *args)
    monkeypatch.setattr(ops, "_call", call)
    runs = []
    for graphs in (False, True, True):
        gm = LlamaModel(mc, "cuda", init="empty").copy_from(cpu_model)
        e = _engine(name, mc, gm, graphs, kv_dtype)
        orig_attn = gm.attention

        def attention(li, qkv, meta, *a, _orig=orig_attn, **k):
            mixed[0] += int(meta.num_decode > 0 and meta.num_prefill_tokens > 0)
            return _orig(li, qkv, meta, *a, **k)
        gm.attention = attention
        runs.append([r.output for r in e.generate(prompts, sp)])
        torch.cuda.synchronize()
    assert runs[0] == runs[1] == runs[2]
    want = {40} if name == "mistral-tiny" else {0, 40}
    assert windows["paged_decode"] == want and windows["paged_prefill"] == want
    assert mixed[0] > 0, "no step had decode rows beside a prefill chunk"
    monkeypatch.setattr(ops, "_call", orig_call)
    assert _teacher_forced_ok(name, cpu_model, prompts, runs[0], kv_dtype) == 24


# ---------------------------------------------------------------------------- bindings

def test_binding_refuses_a_negative_window_and_a_window_with_a_tree():
    c = ac.build("D", 8, 2, 128, [40], device=DEV)
    out = torch.empty(1, 8 * 128, dtype=torch.bfloat16, device=DEV)
    e = torch.empty(0, device=DEV)
    with pytest.raises(RuntimeError, match="window"):
        torch.ops.dgi.paged_decode(out, c.q, c.kc, c.vc, c.bt, c.ctx, e, e, 8, 2, 1, 128, c.scale, None, None, -1)
    torch.ops.dgi.paged_decode(out, c.q, c.kc, c.vc, c.bt, c.ctx, e, e, 8, 2, 1, 128, c.scale, None, None, 8)
    p = ac.build("D", 8, 2, 128, [40], [8], device=DEV)
    outp = torch.empty(8, 8 * 128, dtype=torch.bfloat16, device=DEV)
    tiles = torch.tensor([[0, 0]], dtype=torch.int32, device=DEV)
    tm = ops.tree_mask_ref(torch.tensor([[-1, 0, 0, 1]], dtype=torch.int32))[0].to(DEV)
    tm64 = torch.zeros(1, 64, dtype=torch.int64, device=DEV)
    tm64[:, : tm.shape[-1]] = tm
    with pytest.raises(RuntimeError, match="window"):
        torch.ops.dgi.paged_prefill(outp, p.q, p.kc, p.vc, p.bt, p.cu, p.ctx, tiles, 8, 2, p.scale, None, 0, 128,
                                    None, -1)
    with pytest.raises(RuntimeError, match="tree"):
        torch.ops.dgi.paged_prefill(outp, p.q, p.kc, p.vc, p.bt, p.cu, p.ctx, tiles, 8, 2, p.scale, tm64, 4, 128,
                                    None, 8)
    # each alone is fine
    torch.ops.dgi.paged_prefill(outp, p.q, p.kc, p.vc, p.bt, p.cu, p.ctx, tiles, 8, 2, p.scale, tm64, 4, 128, None, 0)
    torch.ops.dgi.paged_prefill(outp, p.q, p.kc, p.vc, p.bt, p.cu, p.ctx, tiles, 8, 2, p.scale, None, 0, 128, None, 8)
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="window"):
        ops.paged_decode(c.q, c.kc, c.vc, c.bt, c.ctx, 8, 2, c.scale, window=-3)
