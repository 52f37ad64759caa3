"""The exact-answer attention checks test themselves (no GPU).

* The project's fp32 references pass every family's checker, which also pins them to the fp64
  reference of ``attn_cases``.
* Mutants of the fp64 reference, each modelling one slip a kernel change can make (a dropped or
  doubled token, a wrong page, a mask off by one, one wrong rescale factor), are rounded to bf16
  and run through the same checkers.  The full mutant x family matrix of caught / not caught is
  asserted; every mutant is caught by at least one family.
* The stated preconditions (needle margin >= 20 nats, one token moves a count by >= 2x its
  tolerance) hold for every shape the GPU file runs.
"""
import pytest
import torch

import attn_cases as ac
import test_attention_exact_gpu as gpu_file
from dgi import ops

HDS = (128, 64)
DEC_CTXS = [1, 33, 130, 300]                        # 1 / 2 / 5 / 10 tiles, 1 / 1 / 2 / 3 parts of 128
PRE = ([70, 0, 33], [200, 20, 33])                  # cached prefix of 130 keys, an empty sequence, no prefix
TREE_PARENT = torch.tensor([[-1, 0, 0, 1, 1, 2, 3], [-1, 0, 1, 1, 0, 4, 5], [-1, 0, 0, 0, 2, 2, 5]], dtype=torch.int32)
TREE = ([7, 10, 7], [47, 67, 7])                    # prefixes 40 / 57 (+3 plain rows) / 0
COLUMNS = [f"{f}/{k}" for k in ("dec", "pre") for f in ac.FAMILIES] + ["A/tree", "B/tree"]


def _cases(hd):
    nh, nkv = (8, 2) if hd == 128 else (6, 1)
    tm = ops.tree_mask_ref(TREE_PARENT)[0]
    cs = {}
    for f in ac.FAMILIES:
        cs[f"{f}/dec"] = ac.build(f, nh, nkv, hd, DEC_CTXS, bs=16)
        cs[f"{f}/pre"] = ac.build(f, nh, nkv, hd, PRE[1], PRE[0], bs=8)
    for f in "AB":
        cs[f"{f}/tree"] = ac.build(f, nh, nkv, hd, TREE[1], TREE[0], bs=16, tree_mask=tm, tree_n=7)
    return cs


@pytest.fixture(scope="module", params=HDS)
def cases(request):
    return _cases(request.param)


def _fp32_ref(c):
    if c.causal:
        return ops.paged_prefill_ref(c.q, c.kc, c.vc, c.bt, c.cu, c.ctx, c.nh, c.nkv, c.scale, c.tree_mask, c.tree_n)
    return ops.paged_decode_ref(c.q, c.kc, c.vc, c.bt, c.ctx, c.nh, c.nkv, c.scale)


def test_fp32_references_pass_every_family(cases):
    for name, c in cases.items():
        r = ac.check(c, _fp32_ref(c))
        assert r.ok, f"{name}: {r.detail}"


def test_tiled_online_form_of_the_reference_matches_the_direct_one(cases):
    for name, c in cases.items():
        direct, _ = ac.reference(c)
        tiled, _ = ac.reference(c, {"online": _online(c)})
        scale = direct.abs().clamp_min(1e-300)
        assert float(((tiled - direct).abs() / scale).max()) < 1e-9, name


# ---- mutants ---------------------------------------------------------------

def _online(c, **broken):
    return dict(tile=ac.PREFILL_TILE if c.causal else ac.DECODE_TILE, part=None if c.causal else 128, **broken)


def _scale_key(key, factor):
    def f(m, ctx):
        t = key(ctx)
        if t is not None and 0 <= t < ctx:
            m = m.clone()
            m[:, t] *= factor
        return m
    return {"mult": f}


def _swap_pages(ids):
    # first and last page: K and V move together and attention does not care about key order, so
    # decode notices a swap only through the slots past the end of the last, partly filled page
    ids = ids.clone()
    if len(ids) > 1:
        ids[[0, -1]] = ids[[-1, 0]]
    return ids


def _ignore_one_tree_bit(bits):
    # node 3's first non-ancestor below it becomes visible
    i = min(3, len(bits) - 1)
    for a in range(i):
        if not (bits[i] >> a) & 1:
            bits = list(bits)
            bits[i] |= 1 << a
            break
    return bits


MUTANTS = {
    "drop the last token": lambda c: _scale_key(lambda ctx: ctx - 1, 0.0),
    "drop the first token": lambda c: _scale_key(lambda ctx: 0, 0.0),
    "drop the last token of a middle part": lambda c: _scale_key(
        lambda ctx: 255 if ctx > 256 else 127 if ctx > 128 else None, 0.0),
    "count one token twice": lambda c: _scale_key(lambda ctx: ctx // 2, 2.0),
    "swap two block-table entries": lambda c: {"block_table": _swap_pages},
    "read V one slot late": lambda c: {"v_index": lambda t: (t + 1).clamp(max=len(t) - 1)},
    "causal mask < instead of <=": lambda c: {"causal": lambda k, q: k < q},
    "causal mask <= pos + 1": lambda c: {"causal": lambda k, q: k <= q + 1},
    "ignore one tree-mask bit": lambda c: {"tree_bits": _ignore_one_tree_bit},
    "treat tree rows as plain causal": lambda c: {"tree_bits": lambda bits: None},
    "skip one rescale (stale max for one tile)": lambda c: {"online": _online(c, skip_rescale=1)},
    "apply alpha to O but not to l": lambda c: {"online": _online(c, alpha_not_l=True)},
    "combine splits with equal weights": lambda c: {"online": _online(c, equal_splits=True)},
}

# X = the family's checker rejects the mutant, . = it passes (the mutant does not touch what the
# family measures, or does not exist for that kernel: decode has no causal or tree mask, prefill
# has no splits).  Columns: A B C D decode, A B C D prefill, A B tree.
EXPECTED = {
    "drop the last token": "XXXXXXXXXX",
    "drop the first token": "XXXXXXXXXX",
    "drop the last token of a middle part": "XXXXXXXX..",       # the tree contexts have one part
    "count one token twice": ".XXXXXXXXX",                      # doubling a non-needle key: weight e^-20
    "swap two block-table entries": "XXXXXXXXXX",
    "read V one slot late": "XXXXXXXXXX",
    "causal mask < instead of <=": "....XXXXXX",
    "causal mask <= pos + 1": "....XXXXXX",
    "ignore one tree-mask bit": "........XX",
    "treat tree rows as plain causal": "........XX",
    "skip one rescale (stale max for one tile)": "X.XXX.XXX.",  # B: every score is 0, alpha is 1
    "apply alpha to O but not to l": "X.XXX.XXX.",
    "combine splits with equal weights": "XXXX......",
}


def _matrix(cases):
    rows = {}
    for mname, make in MUTANTS.items():
        row = ""
        for col in COLUMNS:
            c = cases[col]
            out = ac.reference(c, make(c))[0].to(torch.bfloat16)
            row += "." if ac.check(c, out).ok else "X"
        rows[mname] = row
    return rows


def _show(rows):
    w = max(len(m) for m in rows)
    head = " " * w + "  " + " ".join(f"{c:>6}" for c in COLUMNS)
    return "\n".join([head] + [f"{m:<{w}}  " + " ".join(f"{x:>6}" for x in r) for m, r in rows.items()])


def test_every_mutant_is_caught(cases):
    rows = _matrix(cases)
    table = _show(rows)
    print("\n" + table)
    missed = [m for m, r in rows.items() if "X" not in r]
    assert not missed, f"not caught by any family: {missed}\n{table}"
    assert rows == EXPECTED, f"mutant x family matrix changed\n{table}"


def test_unbroken_fp64_reference_passes(cases):
    for name, c in cases.items():
        r = ac.check(c, ac.reference(c)[0].to(torch.bfloat16))
        assert r.ok, f"{name}: {r.detail}"


# ---- the stated preconditions, for every shape of the GPU file ---------------

def _gpu_shapes():
    for nh, nkv, hd in gpu_file.DECODE_SHAPES:
        yield nh, nkv, hd, gpu_file.DECODE_CTXS, None, None, 0
    nh, nkv, hd = gpu_file.WIDE_SHAPE
    yield nh, nkv, hd, gpu_file.WIDE_CTXS, None, None, 0
    for nh, nkv, hd in gpu_file.PREFILL_SHAPES:
        for qlens, ctxs in gpu_file.PREFILL_PAIRS:
            yield nh, nkv, hd, ctxs, qlens, None, 0
    for nh, nkv, hd in gpu_file.TREE_SHAPES:
        for n, qlens, ctxs in gpu_file.TREE_CASES:
            yield nh, nkv, hd, ctxs, qlens, gpu_file.tree_masks(n, len(ctxs)), n


@pytest.mark.parametrize("shape", list(_gpu_shapes()), ids=lambda s: f"{s[0]}-{s[1]}-{s[2]}-{'dec' if s[4] is None else s[4]}-{s[6]}")
def test_preconditions_hold_for_the_gpu_shapes(shape):
    nh, nkv, hd, ctxs, qlens, tm, n = shape
    a = ac.build("A", nh, nkv, hd, ctxs, qlens, tree_mask=tm, tree_n=n)
    assert a.min_margin >= ac.MIN_MARGIN, f"needle margin {a.min_margin:.2f} nats"
    assert bool(a.exact.any())
    if qlens is not None and max(qlens) >= 2:
        assert not bool(a.exact.all()), "no must-not-see row"
    b = ac.build("B", nh, nkv, hd, gpu_file.count_ctxs(hd, ctxs) if qlens is None else ctxs, qlens, tree_mask=tm, tree_n=n)
    assert max(b.ctxs) <= (4097 if hd == 128 else 2049)
    sens = ac.count_sensitivity(b)
    assert sens >= 2.0, f"one token moves a count by {sens:.2f}x the tolerance"
