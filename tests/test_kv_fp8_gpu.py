"""FP8 KV cache on the GPU: the e4m3 RoPE writer bit for bit against the reference, both attention
kernels on e4m3 pages through the exact-answer cases of tests/attn_cases.py (unchanged checkers: the
widening is exact, so the bounds derived for bf16 pages hold as they are), byte-exact page movement
and an fp8-KV engine (the CPU side: test_kv_fp8.py)."""
import pytest
import torch

import attn_cases as ac
from dgi import ops
from test_attention_exact_gpu import (BLOCK_SIZES, DECODE_CTXS, PREFILL_CFGS, PREFILL_PAIRS, TREE_CASES, WIDE_CTXS,
                                      WIDE_SHAPE, count_ctxs, tree_masks)

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP8 = torch.float8_e4m3fn
NAN_CODE = 0x7F
PROMPTS = [[1] + list(range(7, 7 + n - 1)) for n in (5, 40, 200, 7)]       # test_fp8_weights_gpu.PROMPTS
DECODE_SHAPES = [(32, 8, 128), (28, 4, 128), (16, 1, 64), (14, 2, 64)]
PREFILL_SHAPES = [(32, 8, 128), (14, 2, 64)]
SCALE_MODES = ("unit", "pow2")


@pytest.fixture(autouse=True, scope="module")
def _native():
    ops.load_native(required=True)


def _scales(nkv, mode, device=DEV):
    """[2, nkv] fp32.  pow2: 2^((h % 5) - 2) for K and 2^(((h + 3) % 5) - 2) for V — a wrong head, or K
    and V swapped, is off by a factor of two at least.  odd: non-power-of-two values."""
    h = torch.arange(nkv, device=device)
    if mode == "unit":
        return torch.ones(2, nkv, device=device)
    if mode == "pow2":
        return torch.stack([torch.exp2(((h % 5) - 2).float()), torch.exp2((((h + 3) % 5) - 2).float())])
    return torch.stack([0.37 + 0.11 * h.float(), 1.9 - 0.13 * h.float()])


def _inverse(scale):
    """The stored inverse, computed once on the host in fp32 (BlockPool.set_kv_scales)."""
    return (torch.ones((), dtype=torch.float32) / scale.cpu()).to(scale.device)


# ----------------------------------------------------------------------------
# writer
# ----------------------------------------------------------------------------

def _writer_case(nh, nkv, hd, rd, mode, T, scale_mode, bs=16, seed=0):
    g = torch.Generator().manual_seed(seed + T)
    nblk = (T + bs - 1) // bs + 3
    width = (nh + 2 * nkv) * hd
    # mostly N(0, 1); a tenth of the entries around 2000 (past 448 * scale for every scale used) and a
    # tenth around 2^-14 (below half the smallest subnormal times the smallest scale)
    x = torch.randn(T, width, generator=g)
    u = torch.rand(T, width, generator=g)
    x = torch.where(u < 0.1, x * 2000.0, torch.where(u > 0.9, x * 2.0 ** -14, x))
    qkv = x.to(torch.bfloat16)
    pos = torch.randint(0, 500, (T,), generator=g, dtype=torch.int32)
    slots = torch.randperm(nblk * bs, generator=g)[:T].to(torch.int32)
    slots[torch.rand(T, generator=g) < 0.1] = -1
    cos_sin = ops.rope_cos_sin(rd, 512, 10000.0)
    scale = _scales(nkv, scale_mode, "cpu")
    return qkv, pos, cos_sin, slots, nblk, scale, _inverse(scale)


WRITER_GEOMS = [(32, 8, 128, 128, 0), (32, 2, 128, 64, 1), (14, 2, 64, 64, 0)]


@pytest.mark.parametrize("T", [1, 7, 300])
@pytest.mark.parametrize("nh,nkv,hd,rd,mode", WRITER_GEOMS)
def test_rope_cache_fp8_bit_exact(nh, nkv, hd, rd, mode, T):
    _writer_check(nh, nkv, hd, rd, mode, T, "pow2")


@pytest.mark.parametrize("nh,nkv,hd,rd,mode", WRITER_GEOMS)
def test_rope_cache_fp8_bit_exact_odd_scales(nh, nkv, hd, rd, mode):
    """Non-power-of-two scales are still exact: both sides multiply by the same stored fp32 inverse."""
    _writer_check(nh, nkv, hd, rd, mode, 300, "odd")


def _writer_check(nh, nkv, hd, rd, mode, T, scale_mode):
    bs = 16
    qkv, pos, cos_sin, slots, nblk, scale, inv = _writer_case(nh, nkv, hd, rd, mode, T, scale_mode)

    def fresh(dev):
        return torch.full((2, nblk, nkv, bs, hd), NAN_CODE, dtype=torch.uint8, device=dev).view(FP8)
    want_kv, want_q = fresh("cpu"), qkv.clone()
    ops.rope_cache_ref(want_q, pos, cos_sin, nh, nkv, hd, slots, want_kv[0], want_kv[1], mode, kv_inv_scale=inv)
    got_kv, got_q = fresh(DEV), qkv.to(DEV)
    ops.rope_cache(got_q, pos.to(DEV), cos_sin.to(DEV), nh, nkv, hd, slots.to(DEV), got_kv[0], got_kv[1], mode,
                   kv_inv_scale=inv.to(DEV))
    torch.cuda.synchronize()
    wk, gk = want_kv.view(torch.uint8), got_kv.cpu().view(torch.uint8)
    assert torch.equal(gk, wk), f"{int((gk != wk).sum())} codes differ"
    assert torch.equal(got_q.cpu().view(torch.int16), want_q.view(torch.int16))
    # the inputs did reach both ends of the format, and every unwritten slot still holds the poison
    written = torch.zeros(nblk * bs, dtype=torch.bool)
    written[slots[slots >= 0].long()] = True
    per_slot = wk.view(2, nblk, nkv, bs, hd).permute(1, 3, 0, 2, 4).reshape(nblk * bs, -1)
    assert bool((per_slot[~written] == NAN_CODE).all())
    if T >= 7:
        live = per_slot[written]
        assert bool(((live & 0x7F) == 0x7E).any()) and bool(((live & 0x7F) == 0).any())
        assert not bool(((live & 0x7F) == NAN_CODE).any())


def test_rope_cache_fp8_rejects_bad_operands():
    qkv = torch.zeros(4, (8 + 4) * 128, dtype=torch.bfloat16, device=DEV)
    pos = torch.zeros(4, dtype=torch.int32, device=DEV)
    cs = ops.rope_cos_sin(128, 16, 10000.0, device=DEV)
    kv8 = torch.zeros(2, 2, 2, 16, 128, dtype=torch.uint8, device=DEV).view(FP8)
    kv16 = torch.zeros(2, 2, 2, 16, 128, dtype=torch.bfloat16, device=DEV)
    ones = torch.ones(2, 2, device=DEV)
    with pytest.raises(RuntimeError):       # fp8 pages without scales
        torch.ops.dgi.rope_cache(qkv, pos, cs, 8, 2, 128, pos, kv8[0], kv8[1], 0, None)
    with pytest.raises(RuntimeError):       # scales of the wrong shape
        torch.ops.dgi.rope_cache(qkv, pos, cs, 8, 2, 128, pos, kv8[0], kv8[1], 0, torch.ones(2, 3, device=DEV))
    with pytest.raises(RuntimeError):       # scales with bf16 pages
        torch.ops.dgi.rope_cache(qkv, pos, cs, 8, 2, 128, pos, kv16[0], kv16[1], 0, ones)
    with pytest.raises(RuntimeError):       # K and V of different dtypes
        torch.ops.dgi.rope_cache(qkv, pos, cs, 8, 2, 128, pos, kv8[0], kv16[1], 0, ones)
    with pytest.raises(RuntimeError):
        torch.ops.dgi.paged_decode(qkv[:, :1024], qkv, kv8[0].view(torch.uint8), kv8[1].view(torch.uint8),
                                   torch.zeros(4, 1, dtype=torch.int32, device=DEV), pos,
                                   torch.empty(0, device=DEV), torch.empty(0, device=DEV), 8, 2, 1, 128, 1.0, None, ones)


# ----------------------------------------------------------------------------
# attention on e4m3 pages, judged by the unchanged exact-answer checkers
# ----------------------------------------------------------------------------

def _to_fp8(c, scale_mode, every_code=False):
    """Round the case's K/V pool to e4m3 codes for the chosen scales and replace c.kc / c.vc by the
    dequantised bf16 (what the checkers and the fp64 reference then see).  NaN stays NaN (code 0x7F).
    Returns (k codes, v codes, scales)."""
    scale = _scales(c.nkv, scale_mode)
    inv = _inverse(scale)
    codes = []
    for j, pool in enumerate((c.kc, c.vc)):
        q = ops.quantize_kv_ref(pool.transpose(1, 2), inv[j]).transpose(1, 2).contiguous()     # [blocks, nkv, bs, hd]
        if every_code:
            # every finite code somewhere among the live values: overwrite the finite entries cyclically
            b = q.view(torch.uint8)
            fin = (b & 0x7F) != NAN_CODE
            allc = torch.tensor([x for x in range(256) if x & 0x7F != NAN_CODE], dtype=torch.uint8, device=b.device)
            # small magnitudes only for K (|code value| <= 4) so the scores stay in softmax range
            if j == 0:
                allc = allc[((allc & 0x7F) <= 0x48)]
            b[fin] = allc[(torch.arange(int(fin.sum()), device=b.device) * 7) % len(allc)]
        nan = (q.view(torch.uint8) & 0x7F) == NAN_CODE
        q.view(torch.uint8)[nan] = NAN_CODE
        deq = ops.dequantize_kv_ref(q.transpose(1, 2), scale[j]).transpose(1, 2)
        assert torch.equal(deq.to(torch.bfloat16).float().nan_to_num(7e7), deq.nan_to_num(7e7))   # exact in bf16
        (c.kc if j == 0 else c.vc).copy_(deq.to(torch.bfloat16))
        codes.append(q)
    c.ref_cache = None
    return codes[0], codes[1], scale


def _report(failures, worst, family, kernel):
    print(f"RATIO fp8 {family} {kernel} {worst:.4f}")
    assert not failures, "\n".join(failures)


def _decode_plans(c, k8, v8, sc):
    """Every launch plan of test_attention_exact_gpu._decode_plans, on the e4m3 pages."""
    B, nh, nkv, hd = len(c.ctxs), c.nh, c.nkv, c.hd
    args = (c.q, k8, v8, c.bt, c.ctx, nh, nkv, c.scale)
    mx = max(c.ctxs)
    yield "one split", ops.paged_decode(*args, 1, 1 << 20, kv_scale=sc)
    splits, part = ops.decode_split_plan(B, mx, nkv)
    yield f"split plan {splits}x{part}", ops.paged_decode(*args, splits, part, kv_scale=sc)
    yield "part 128, spare splits", ops.paged_decode(*args, (mx + 127) // 128 + 3, 128, kv_scale=sc)
    ws2 = (torch.empty(B * nh * splits * hd, device=DEV), torch.empty(B * nh * splits, device=DEV))
    yield "reduce kernel", ops.paged_decode(*args, splits, part, workspace=ws2, kv_scale=sc)
    for S, mn in ac.DEVICE_PLANS:
        ws = (torch.empty(B * nh * S * hd, device=DEV), torch.empty(B * nh * S, device=DEV),
              torch.zeros(B * nkv, dtype=torch.int32, device=DEV))
        for rep in range(2):
            yield f"device plan S={S} min={mn} run {rep}", ops.paged_decode(*args, S, -mn, workspace=ws, kv_scale=sc)
        assert int(ws[2].abs().sum()) == 0, f"ticket counters not back to zero (S={S}, min={mn})"


def _decode_case(family, nh, nkv, hd, ctxs, scale_mode, bs=16, plans=_decode_plans, every_code=False):
    c = ac.build(family, nh, nkv, hd, count_ctxs(hd, ctxs) if family == "B" else ctxs, bs=bs, device=DEV)
    k8, v8, sc = _to_fp8(c, scale_mode, every_code)
    failures, worst = [], 0.0
    for name, out in plans(c, k8, v8, sc):
        r = ac.check(c, out)
        worst = max(worst, r.ratio)
        if not r.ok:
            failures.append(f"{name}: {r.detail}")
    return failures, worst


def test_family_a_values_are_exact_in_e4m3():
    c = ac.build("A", 32, 8, 128, [129], bs=16, device=DEV)
    k0, v0 = c.kc.clone(), c.vc.clone()
    _to_fp8(c, "pow2")
    assert torch.equal(c.kc.nan_to_num(9.0), k0.nan_to_num(9.0)) and torch.equal(c.vc.nan_to_num(9.0), v0.nan_to_num(9.0))


@pytest.mark.parametrize("scale_mode", SCALE_MODES)
@pytest.mark.parametrize("family", ac.FAMILIES)
@pytest.mark.parametrize("nh,nkv,hd", DECODE_SHAPES)
def test_decode_fp8(nh, nkv, hd, family, scale_mode):
    _report(*_decode_case(family, nh, nkv, hd, DECODE_CTXS, scale_mode), family, "decode")


@pytest.mark.parametrize("scale_mode", SCALE_MODES)
@pytest.mark.parametrize("family", ac.FAMILIES)
@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_decode_fp8_block_sizes(bs, family, scale_mode):
    _report(*_decode_case(family, 32, 8, 128, DECODE_CTXS, scale_mode, bs=bs), family, "decode")


@pytest.mark.parametrize("scale_mode", SCALE_MODES)
@pytest.mark.parametrize("family", ac.FAMILIES)
def test_decode_fp8_40_sequences(family, scale_mode):
    def plans(c, k8, v8, sc):
        args = (c.q, k8, v8, c.bt, c.ctx, c.nh, c.nkv, c.scale)
        yield "one split (4 waves)", ops.paged_decode(*args, 1, 1 << 20, kv_scale=sc)
        yield "part 128", ops.paged_decode(*args, (max(c.ctxs) + 127) // 128, 128, kv_scale=sc)
    _report(*_decode_case(family, *WIDE_SHAPE, WIDE_CTXS, scale_mode, plans=plans), family, "decode")


def _prefill_case(monkeypatch, family, nh, nkv, hd, pairs, scale_mode, bs=16, cfgs=PREFILL_CFGS, tree=None,
                  every_code=False):
    failures, worst = [], 0.0
    for qlens, ctxs in pairs:
        tm, n = (tree_masks(tree, len(ctxs)), tree) if tree else (None, 0)
        c = ac.build(family, nh, nkv, hd, ctxs, qlens, bs=bs, device=DEV, tree_mask=tm, tree_n=n)
        k8, v8, sc = _to_fp8(c, scale_mode, every_code)
        for tile, db in cfgs:
            monkeypatch.setattr(ops, "PREFILL_TILE", tile)
            monkeypatch.setattr(ops, "PREFILL_DB", db)
            out = ops.paged_prefill(c.q, k8, v8, c.bt, c.cu, c.ctx, nh, nkv, c.scale, tree_mask=c.tree_mask,
                                    tree_n=c.tree_n, kv_scale=sc)
            r = ac.check(c, out)
            worst = max(worst, r.ratio)
            if not r.ok:
                failures.append(f"qlens {qlens} ctxs {ctxs} tile {tile} db {db}: {r.detail}")
    return failures, worst


@pytest.mark.parametrize("scale_mode", SCALE_MODES)
@pytest.mark.parametrize("family", ac.FAMILIES)
@pytest.mark.parametrize("nh,nkv,hd", PREFILL_SHAPES)
def test_prefill_fp8(nh, nkv, hd, family, scale_mode, monkeypatch):
    _report(*_prefill_case(monkeypatch, family, nh, nkv, hd, PREFILL_PAIRS, scale_mode), family, "prefill")


@pytest.mark.parametrize("scale_mode", SCALE_MODES)
@pytest.mark.parametrize("family", ac.FAMILIES)
@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_prefill_fp8_block_sizes(bs, family, scale_mode, monkeypatch):
    _report(*_prefill_case(monkeypatch, family, 32, 8, 128, PREFILL_PAIRS, scale_mode, bs=bs), family, "prefill")


@pytest.mark.parametrize("scale_mode", SCALE_MODES)
@pytest.mark.parametrize("family", ["A", "B"])
@pytest.mark.parametrize("n,qlens,ctxs", TREE_CASES)
@pytest.mark.parametrize("nh,nkv,hd", [(32, 8, 128), (14, 2, 64)])
def test_prefill_fp8_tree_mask(nh, nkv, hd, n, qlens, ctxs, family, scale_mode, monkeypatch):
    _report(*_prefill_case(monkeypatch, family, nh, nkv, hd, [(qlens, ctxs)], scale_mode, tree=n), family, "tree")


@pytest.mark.parametrize("nh,nkv,hd", [(32, 8, 128), (14, 2, 64)])
def test_attention_fp8_every_code(nh, nkv, hd, monkeypatch):
    """Family D's bound with K and V holding all 254 finite codes (K: every code up to |4|, both signs,
    subnormals and zeros included): an fnuz decode, a dropped subnormal or a lost sign misses it."""
    _report(*_decode_case("D", nh, nkv, hd, [1, 33, 257, 1000], "pow2", every_code=True), "D", "decode every code")
    _report(*_prefill_case(monkeypatch, "D", nh, nkv, hd, [([129, 0, 33], [129, 50, 600])], "pow2", every_code=True),
            "D", "prefill every code")


# ----------------------------------------------------------------------------
# page movement
# ----------------------------------------------------------------------------

@pytest.mark.parametrize("hd", [64, 128])
def test_kv_page_movement_fp8_byte_exact(hd):
    from dgi.spec.eagle3 import kv_slot_copy
    L, NB, nkv, bs = 3, 12, 2, 16
    g = torch.Generator().manual_seed(hd)
    raw = torch.randint(0, 256, (L, 2, NB, nkv, bs, hd), generator=g, dtype=torch.uint8)
    kv = raw.to(DEV).view(FP8)
    ids = torch.tensor([5, 1, 9, 2], dtype=torch.int32, device=DEV)
    for block_major in (False, True):
        buf = ops.kv_gather(kv, ids, block_major=block_major)
        assert buf.dtype == FP8
        want = raw[:, :, ids.cpu().long()]
        if block_major:
            want = want.permute(2, 0, 1, 3, 4, 5)
        assert torch.equal(buf.cpu().view(torch.uint8), want.contiguous())
        dst = torch.zeros_like(raw).to(DEV).view(FP8)
        ops.kv_scatter(dst, ids, buf, block_major=block_major)
        got = dst.cpu().view(torch.uint8)
        assert torch.equal(got[:, :, ids.cpu().long()], raw[:, :, ids.cpu().long()])
        rest = torch.ones(NB, dtype=torch.bool)
        rest[ids.cpu().long()] = False
        assert not got[:, :, rest].any()
    cp = raw.clone().to(DEV).view(FP8)
    src = torch.tensor([5, 1], dtype=torch.int32, device=DEV)
    dstb = torch.tensor([7, 8], dtype=torch.int32, device=DEV)
    ops.kv_copy(cp, src, dstb)
    want = raw.clone()
    want[:, :, [7, 8]] = raw[:, :, [5, 1]]
    assert torch.equal(cp.cpu().view(torch.uint8), want)
    sc = raw.clone().to(DEV).view(FP8)
    s_src = torch.tensor([3 * bs + 2, 5 * bs + 15, 17], device=DEV)
    s_dst = torch.tensor([4 * bs + 0, 17, 9 * bs + 1], device=DEV)
    kv_slot_copy(sc, s_src, s_dst, bs)
    want = raw.clone().view(L * 2, NB, nkv, bs, hd)
    vals = raw.view(L * 2, NB, nkv, bs, hd)[:, s_src.cpu() // bs, :, s_src.cpu() % bs]
    want[:, s_dst.cpu() // bs, :, s_dst.cpu() % bs] = vals
    assert torch.equal(sc.cpu().view(torch.uint8), want.view_as(raw))


# ----------------------------------------------------------------------------
# engine
# ----------------------------------------------------------------------------

def _spy(monkeypatch):
    calls = []
    orig = ops._call

    def call(name, *args):
        calls.append((name, args))
        return orig(name, *args)
    monkeypatch.setattr(ops, "_call", call)
    return calls


def _teacher_forced_ok(name, f32_model, prompts, gpu_outs, rel=0.03, abs_=0.02):
    """test_fp8_weights_gpu._teacher_forced_ok with the reference engine on an fp8 KV pool: every token
    the GPU chose is an argmax of the fp32 CPU model's logits for the same prefix, up to the project's
    bf16 tolerance."""
    from dgi.engine import EngineConfig, LLMEngine
    from dgi.sched.request import SamplingParams
    ref = LLMEngine(EngineConfig(model=name, device="cpu", dtype=torch.float32, num_blocks=256, max_num_seqs=8,
                                 max_model_len=512, max_num_batched_tokens=256, use_graphs=False,
                                 enable_prefix_caching=False, kv_dtype="fp8"), model_cfg=f32_model.cfg, model=f32_model)
    assert ref.pool.dtype == FP8
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


def _assert_fp8_path(calls):
    names = [n for n, _ in calls]
    assert {"rope_cache", "paged_decode", "paged_prefill"} <= set(names)
    assert "mfma_gemm_norm_rope" not in names
    for n, a in calls:
        if n == "fused_skinny":
            assert a[9] != 2, "a KV-writing fused_skinny epilogue ran on an fp8 pool"
        if n == "rope_cache":
            assert a[7].dtype == FP8 and a[10] is not None


@pytest.mark.parametrize("weight_quant", [None, "fp8"])
def test_fp8_kv_engine_teacher_forced(weight_quant, monkeypatch):
    from dgi.engine import EngineConfig, LLMEngine
    from dgi.models.config import get_config
    from dgi.models.llama import QUANT_SLOTS, LlamaModel
    from dgi.ops import Fp8Weight
    from dgi.sched.request import SamplingParams
    name = "llama-tiny-hd128"
    mc = get_config(name)
    src = LlamaModel(mc, "cpu", seed=5)
    sp = SamplingParams(max_tokens=10, temperature=0.0, ignore_eos=True)
    calls = _spy(monkeypatch)
    outs, models = {}, {}
    for graphs in (False, True):
        gm = LlamaModel(mc, "cuda", init="empty").copy_from(src)
        eng = LLMEngine(EngineConfig(model=name, device="cuda", num_blocks=256, max_num_seqs=8, max_model_len=512,
                                     max_num_batched_tokens=256, use_graphs=graphs, kv_dtype="fp8",
                                     weight_quant=weight_quant), model_cfg=mc, model=gm)
        assert eng.pool.dtype == FP8 and eng.pool.kv.dtype == FP8 and gm.kv_fp8
        del calls[:]
        outs[graphs] = [r.output for r in eng.generate(PROMPTS, sp)]
        _assert_fp8_path(calls)
        models[graphs] = gm
    assert all(len(o) == 10 for o in outs[False])
    f32 = LlamaModel(mc, "cpu", torch.float32, init="empty").copy_from(src)
    if weight_quant:
        for L, Lq in zip(f32.layers, models[False].layers):
            for k in QUANT_SLOTS:
                fw = getattr(Lq, k)
                getattr(L, k).copy_(Fp8Weight(fw.q.cpu(), fw.scale.cpu()).dequant(torch.float32))
    assert _teacher_forced_ok(name, f32, PROMPTS, outs[False]) == 40
    assert outs[True] == outs[False]


def test_fp8_kv_engine_host_tier_swap():
    """A pool too small for every running sequence with a host tier (test_host_tier's recipe): victims'
    e4m3 pages are swapped out and back, no prompt token is prefilled twice, and every token still
    passes the teacher-forced check."""
    from dgi.engine import EngineConfig, LLMEngine
    from dgi.models.config import get_config
    from dgi.models.llama import LlamaModel
    from dgi.sched.request import SamplingParams
    name = "llama-tiny-hd128"
    mc = get_config(name)
    src = LlamaModel(mc, "cpu", seed=5)
    g = torch.Generator().manual_seed(3)
    prompts = [torch.randint(5, 500, (20 + 3 * i,), generator=g).tolist() for i in range(6)]
    sp = SamplingParams(max_tokens=12, temperature=0.0, ignore_eos=True)
    gm = LlamaModel(mc, "cuda", init="empty").copy_from(src)
    # 13 pages hold the prompts, 18 the finished sequences; 14 usable pages force preemption
    eng = LLMEngine(EngineConfig(model=name, device="cuda", num_blocks=15, max_num_seqs=6, max_model_len=256,
                                 max_num_batched_tokens=256, use_graphs=False, kv_dtype="fp8",
                                 enable_prefix_caching=False, host_kv_gb=0.05), model_cfg=mc, model=gm)
    outs = [r.output for r in eng.generate(prompts, sp)]
    assert eng.host_tier.host.dtype == FP8
    st = eng.scheduler.stats()
    assert st["preemptions"] > 0 and st["swapped_out"] == st["preemptions"] == st["swapped_in"], st
    assert eng.stats["prefill_tokens"] == sum(len(p) for p in prompts)
    f32 = LlamaModel(mc, "cpu", torch.float32, init="empty").copy_from(src)
    assert _teacher_forced_ok(name, f32, prompts, outs) == 72
