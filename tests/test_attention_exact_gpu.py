"""paged_decode / paged_prefill against inputs whose answer is known exactly (tests/attn_cases.py).

Run on an MI355X (``pytest -m gpu``).  Every family runs through every launch plan, block size
and tile configuration the kernels have; a single wrong token, page, mask bit or rescale factor
moves the output far outside the tolerance (tests/test_attention_exact_cpu.py proves that on
broken references).  Each test prints its worst error / tolerance ratio (``RATIO ...`` lines,
``pytest -s``); the ratios are recorded in profiles/attn_exact/README.md.
"""
import random

import pytest
import torch

import attn_cases as ac
from dgi import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"

DECODE_SHAPES = [(32, 8, 128), (64, 8, 128), (8, 8, 128), (28, 4, 128), (16, 1, 128), (16, 1, 64), (14, 2, 64)]
DECODE_CTXS = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 257, 1000, 2049, 4097]
# 40 sequences in one launch: B * nkv > 128, so one split runs the 4-wave kernel
WIDE_SHAPE = (32, 8, 128)
WIDE_CTXS = [1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 95, 96, 97, 127, 128, 129, 130, 159, 160, 161, 191,
             192, 193, 255, 256, 257, 300, 383, 384, 385, 511, 512, 513, 777, 1023, 1025]
PREFILL_SHAPES = [(32, 8, 128), (8, 1, 128), (28, 4, 128), (32, 8, 64), (14, 2, 64)]
PREFILL_CFGS = [(128, 1), (128, 0), (256, 1), (256, 0)]            # (PREFILL_TILE, PREFILL_DB)
PREFILL_PAIRS = [([1], [1]), ([64], [64]), ([65], [65]), ([129, 0, 33], [129, 50, 600]), ([127], [127 + 64]),
                 ([128], [128 + 63]), ([257], [1000]), ([300, 77], [1000, 77])]
BLOCK_SIZES = [8, 16, 32, 64]
TREE_SHAPES = [(32, 8, 128), (14, 2, 64)]
# (draft nodes, qlens, ctxs): cached prefixes of 40, 57 (the tree straddles a 64-key tile), 0,
# and 57 with 3 plain causal rows in front of the tree
TREE_CASES = [(7, [7, 7, 7, 10], [47, 64, 7, 67]), (64, [64, 64, 64], [104, 121, 64])]


def count_ctxs(hd, ctxs):
    """Family B keeps one token worth >= 2x the tolerance: contexts up to 2049 at head dim 64."""
    return [min(c, 2049) for c in ctxs] if hd == 64 else list(ctxs)


def tree_masks(n, B):
    """Ancestor masks of B seeded random draft trees of n nodes; the last node of the first tree
    hangs off a chain through node n - 2, so with n = 64 bit 63 is set next to low bits."""
    rng = random.Random(n)
    par = [[-1] + [rng.randrange(0, i) for i in range(1, n)] for _ in range(B)]
    if n > 2:
        par[0][n - 1] = n - 2
    return ops.tree_mask_ref(torch.tensor(par, dtype=torch.int32))[0]


@pytest.fixture(autouse=True, scope="module")
def _native():
    ops.load_native(required=True)
    assert len(set(WIDE_CTXS)) == 40


def _report(failures, worst, family, kernel):
    print(f"RATIO {family} {kernel} {worst:.4f}")
    assert not failures, "\n".join(failures)


def _decode_plans(c):
    """(plan name, output) for every launch plan test_kernels_gpu._paged_decode_case drives."""
    B, nh, nkv, hd = len(c.ctxs), c.nh, c.nkv, c.hd
    args = (c.q, c.kc, c.vc, c.bt, c.ctx, nh, nkv, c.scale)
    mx = max(c.ctxs)
    yield "one split", ops.paged_decode(*args, 1, 1 << 20)
    splits, part = ops.decode_split_plan(B, mx, nkv)
    yield f"split plan {splits}x{part}", ops.paged_decode(*args, splits, part)
    yield "part 128, spare splits", ops.paged_decode(*args, (mx + 127) // 128 + 3, 128)
    ws2 = (torch.empty(B * nh * splits * hd, device=DEV), torch.empty(B * nh * splits, device=DEV))
    yield "reduce kernel", ops.paged_decode(*args, splits, part, workspace=ws2)
    for S, mn in ac.DEVICE_PLANS:
        ws = (torch.empty(B * nh * S * hd, device=DEV), torch.empty(B * nh * S, device=DEV),
              torch.zeros(B * nkv, dtype=torch.int32, device=DEV))
        for rep in range(2):
            yield f"device plan S={S} min={mn} run {rep}", ops.paged_decode(*args, S, -mn, workspace=ws)
        assert int(ws[2].abs().sum()) == 0, f"ticket counters not back to zero (S={S}, min={mn})"


def _decode_case(family, nh, nkv, hd, ctxs, bs=16, plans=_decode_plans):
    c = ac.build(family, nh, nkv, hd, count_ctxs(hd, ctxs) if family == "B" else ctxs, bs=bs, device=DEV)
    failures, worst = [], 0.0
    for name, out in plans(c):
        r = ac.check(c, out)
        worst = max(worst, r.ratio)
        if not r.ok:
            failures.append(f"{name}: {r.detail}")
    return failures, worst


@pytest.mark.parametrize("family", ac.FAMILIES)
@pytest.mark.parametrize("nh,nkv,hd", DECODE_SHAPES)
def test_decode(nh, nkv, hd, family):
    _report(*_decode_case(family, nh, nkv, hd, DECODE_CTXS), family, "decode")


@pytest.mark.parametrize("family", ac.FAMILIES)
@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_decode_block_sizes(bs, family):
    _report(*_decode_case(family, 32, 8, 128, DECODE_CTXS, bs=bs), family, "decode")


@pytest.mark.parametrize("family", ac.FAMILIES)
def test_decode_40_sequences(family):
    def plans(c):
        args = (c.q, c.kc, c.vc, c.bt, c.ctx, c.nh, c.nkv, c.scale)
        yield "one split (4 waves)", ops.paged_decode(*args, 1, 1 << 20)
        yield "part 128", ops.paged_decode(*args, (max(c.ctxs) + 127) // 128, 128)
    _report(*_decode_case(family, *WIDE_SHAPE, WIDE_CTXS, plans=plans), family, "decode")


def _prefill_case(monkeypatch, family, nh, nkv, hd, pairs, bs=16, cfgs=PREFILL_CFGS, tree=None):
    failures, worst = [], 0.0
    for qlens, ctxs in pairs:
        tm, n = (tree_masks(tree, len(ctxs)), tree) if tree else (None, 0)
        c = ac.build(family, nh, nkv, hd, ctxs, qlens, bs=bs, device=DEV, tree_mask=tm, tree_n=n)
        for tile, db in cfgs:
            monkeypatch.setattr(ops, "PREFILL_TILE", tile)
            monkeypatch.setattr(ops, "PREFILL_DB", db)
            out = ops.paged_prefill(c.q, c.kc, c.vc, c.bt, c.cu, c.ctx, nh, nkv, c.scale, tree_mask=c.tree_mask,
                                    tree_n=c.tree_n)
            r = ac.check(c, out)
            worst = max(worst, r.ratio)
            if not r.ok:
                failures.append(f"qlens {qlens} ctxs {ctxs} tile {tile} db {db}: {r.detail}")
    return failures, worst


@pytest.mark.parametrize("family", ac.FAMILIES)
@pytest.mark.parametrize("nh,nkv,hd", PREFILL_SHAPES)
def test_prefill(nh, nkv, hd, family, monkeypatch):
    _report(*_prefill_case(monkeypatch, family, nh, nkv, hd, PREFILL_PAIRS), family, "prefill")


@pytest.mark.parametrize("family", ac.FAMILIES)
@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_prefill_block_sizes(bs, family, monkeypatch):
    _report(*_prefill_case(monkeypatch, family, 32, 8, 128, PREFILL_PAIRS, bs=bs), family, "prefill")


@pytest.mark.parametrize("family", ["A", "B"])
@pytest.mark.parametrize("n,qlens,ctxs", TREE_CASES)
@pytest.mark.parametrize("nh,nkv,hd", TREE_SHAPES)
def test_prefill_tree_mask(nh, nkv, hd, n, qlens, ctxs, family, monkeypatch):
    _report(*_prefill_case(monkeypatch, family, nh, nkv, hd, [(qlens, ctxs)], tree=n), family, "tree")
