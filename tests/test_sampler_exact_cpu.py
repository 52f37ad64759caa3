"""The exact-answer sampler / top-k / tree checks test themselves (no GPU).

* The generators of tests/sampler_cases.py satisfy their own conditions: at most 1 % of a case's
  sampled rows are non-decisive under the float64 scores, every filtered row keeps the mass
  condition >= 1e-3 away from flipping, cut values are separated, and the recorded fp32-vs-fp64
  gap (from which ``DELTA`` follows) is the measured one.
* The CPU paths of ``ops.sample``, ``ops.topkp_threshold``, ``ops.topk``, ``ops.topk_logprobs``,
  ``ops.tree_mask`` and ``ops.tree_verify`` pass the comparators the GPU file uses.
* Kernel models with one slip each are rejected by at least one case, for the reason the slip's
  name states.
* ``gumbel_uniform`` lies strictly inside (0, 1).
"""
import pytest
import torch

import sampler_cases as sc
from dgi import ops
from test_ops_cpu import _brute_threshold


def _all_sample_cases():
    return sc.sample_cases() + sc.u1_cases() + [sc.k1_case()]


def _tie_cases():
    return [sc.greedy_tie_case(V, dt) for V in (1023, 4099, 24571) for dt in sc.DTYPES]


# ---- the uniform --------------------------------------------------------------------------------

def test_uniform_from_hash_is_strictly_inside_the_unit_interval():
    h = torch.tensor([0, 0xFFFFFFFF, 0xFFFFFF00, 0xFFFFFE00, 0x80000000, 0x7FFFFFFF, 1 << 9], dtype=torch.long)
    u = ops._uniform_from_hash(h)
    assert u.dtype == torch.float32
    assert bool((u > 0).all()) and bool((u < 1).all()), u.tolist()
    assert float(u[0]) == 2.0 ** -24 and float(u[1]) == 1 - 2.0 ** -24
    # every step is exact in fp32: equal to the dyadic computed in float64
    assert torch.equal(u.double(), ((h >> 9).double() + 0.5) / 8388608.0)
    assert bool(torch.isfinite(-torch.log(-torch.log(u))).all())


def test_the_eight_pairs_that_drew_one_now_draw_inside_the_interval():
    for seed, tok in sc.U1_PAIRS:
        sd = torch.tensor([seed])
        h = int(sc.hash_bits(sd, 0, sc.U1_V)[0, tok])
        assert h >> 8 == (1 << 24) - 1                    # why the 24-bit draw rounded to 1.0f
        assert float((torch.tensor(float(h >> 8)) + 0.5) * (1.0 / 16777216.0)) == 1.0
        u = ops.gumbel_uniform(sd, 0, sc.U1_V, 1)
        assert 0.0 < float(u[0, tok]) < 1.0
        assert 0.0 < float(u.min()) and float(u.max()) < 1.0
        assert torch.equal(u.double(), sc.uniform64(sd, 0, sc.U1_V))


# ---- conditions of the generators ------------------------------------------------------------------

def test_fp32_gap_is_the_recorded_one():
    worst = 0.0
    for c in _all_sample_cases():
        rows = c.temps > 1e-5
        if bool(rows.any()):
            d = (sc.noisy32(c.logits, c.temps, c.seeds, c.step).double() - c.noisy())[rows]
            worst = max(worst, float(d.abs().max()))
    print(f"RATIO fp32-vs-fp64 gap {worst:.3e} recorded {sc.FP32_GAP:.3e} delta {sc.DELTA:.3e}")
    assert 0.95 * sc.FP32_GAP <= worst <= sc.FP32_GAP
    assert sc.DELTA == 16 * sc.FP32_GAP


def test_non_decisive_rows_stay_under_the_cap():
    total = 0
    for c in _all_sample_cases():
        n = c.non_decisive()
        total += n
        assert n <= sc.MAX_NON_DECISIVE * c.sampled_rows(), (c.name, n, c.sampled_rows())
    print(f"COUNT non-decisive rows {total}")


def test_filtered_rows_keep_their_margins():
    for c in _all_sample_cases():
        if c.filt:
            for b, t in enumerate(c.thresh_refs()):
                assert t.gap >= sc.MIN_GAP and t.sep > 4 * sc.SEARCH_WIDTH, (c.name, b, t)


def _per_element_threshold(row, T, k, p):
    """``test_ops_cpu._brute_threshold`` restated over a V x V table in float64 (the Python loops
    take 30 s at V = 1000): every element is judged on its own, no sort, no distinct values."""
    x = torch.tensor(row, dtype=torch.float64)
    gt = x[None, :] > x[:, None]                              # gt[v, u] = u > v
    e = torch.exp((x - x.max()) / T)
    in_k = gt.sum(1) < k
    kept = in_k & ((gt * e[None, :]).sum(1) <= p * e[in_k].sum())
    return float(x[kept].min()) if int(kept.sum()) < len(row) else sc.NEG_INF


@pytest.mark.parametrize("dtype", sc.DTYPES)
@pytest.mark.parametrize("V", sc.THRESH_V)
def test_threshold_cases_cover_what_they_name(V, dtype):
    c = sc.thresh_case(V, dtype)                              # the generator asserts gap and separation
    by = dict(zip(c.rows, range(len(c.rows))))
    ref = c.ref
    b = by["top-k only, ties straddle the cut"]
    assert ref[b].kept == int(c.top_k[b]) + 2 and ref[b].thresh > sc.NEG_INF
    b = by["k = 1"]
    assert ref[b].thresh == float(c.logits[b].double().max())
    b = by["k = V - 1"]
    assert ref[b].kept == V - 1
    b = by["top-p keeps the maximum only"]
    assert ref[b].thresh == float(c.logits[b].double().max())
    for name in ("constant row", "greedy row", "no filter", "greedy row, filter off"):
        assert ref[by[name]].thresh == sc.NEG_INF
    for name in ("k > V, top-p", "k = V, top-p", "-inf tail, top-k then top-p", "-inf tail, k above the finite count",
                 "top-p cut inside the top-k set", "top-p only, 12 values"):
        assert sc.NEG_INF < ref[by[name]].thresh and ref[by[name]].gap < float("inf")
    if V <= 4099:                                             # the literal per-element definition
        for b in range(len(c.rows)):
            row = [v for v in c.logits[b].double().tolist() if v > sc.NEG_INF]
            T, k = float(c.temps[b]), int(c.top_k[b])
            if T <= 1e-5:
                continue
            want = _per_element_threshold(row, T, k if k > 0 else 10 ** 9, float(c.top_p[b]))
            assert ref[b].thresh == want, (c.rows[b], ref[b], want)
            if V <= 100:                                      # ... which is test_ops_cpu's, as a V x V table
                assert want == _brute_threshold(row, T, k if k > 0 else 10 ** 9, float(c.top_p[b]))


# ---- the CPU paths pass the comparators -------------------------------------------------------------

def test_cpu_sample_passes_the_pick_comparator():
    for c in _all_sample_cases() + _tie_cases():
        picks = ops.sample(c.logits, **c.kwargs())
        bad = sc.check_sample(c, picks)
        assert not bad, "\n".join(bad)
        assert not sc.check_sample(c, sc.kernel_model(c)), c.name
    for c in sc.u1_cases():                                   # not the planted id, whatever else holds
        picks = ops.sample(c.logits, **c.kwargs()).tolist()
        assert all(p != sc.U1_PAIRS[b % 8][1] for b, p in enumerate(picks))
        assert all(sc.pick_ok(p, c.noisy()[b], sc.NEG_INF, sc.DELTA, c.logits[b]) for b, p in enumerate(picks))


@pytest.mark.parametrize("dtype", sc.DTYPES)
@pytest.mark.parametrize("V", sc.THRESH_V)
def test_cpu_threshold_is_the_reference_bit_for_bit(V, dtype):
    c = sc.thresh_case(V, dtype)
    th = ops.topkp_threshold(c.logits, c.temps, c.top_k, c.top_p)
    for b, name in enumerate(c.rows):
        assert float(th[b]) == c.ref[b].thresh, (c.name, name, float(th[b]), c.ref[b])
    lg, T, k, p, ref, _ = sc.superset_case()
    assert float(ops.topkp_threshold(lg, T, k, p)[0]) == ref


@pytest.mark.parametrize("dtype", sc.DTYPES)
@pytest.mark.parametrize("V", sc.TOPK_V)
def test_cpu_topk_is_the_stable_sort(V, dtype):
    logits, names = sc.topk_rows(V, dtype)
    for k in sc.TOPK_K:
        v, i = ops.topk(logits, k)
        rv, ri = sc.topk_ref(logits, k)
        assert torch.equal(i, ri) and torch.equal(v.double(), rv), (V, k)
    assert ops.topk(logits[2:3], 8)[1].tolist() == [list(range(8))]          # the constant row
    with pytest.raises(ValueError):
        ops.topk(logits, V + 1)
    with pytest.raises(ValueError):
        ops.topk_logprobs(logits, V + 1)


@pytest.mark.parametrize("V", sc.TKL_V)
def test_cpu_topk_logprobs_match_float64(V):
    logits, names = sc.topk_rows(V, torch.bfloat16, chunk_ties=(2047, 2048))
    lp = sc.logprobs64(logits)
    for k in sc.TKL_K:
        v, i = ops.topk_logprobs(logits, k)
        _, ri = sc.topk_ref(logits, k)
        assert torch.equal(i, ri), (V, k)
        torch.testing.assert_close(v.double(), lp.gather(1, ri), atol=2e-5, rtol=1e-5)


def test_cpu_tree_ops_agree_with_the_brute_force_walk():
    for c in sc.tree_cases():
        anc, depth, acc, path, toks = sc.brute_tree(c)
        for fm in (ops.tree_mask_ref, ops.tree_mask):
            a, d = fm(c.parent)
            assert torch.equal(a, anc) and torch.equal(d, depth), c.name
        for fv in (ops.tree_verify_ref, ops.tree_verify):
            r = fv(c.parent, c.draft, c.target, anc, depth, c.max_path)
            assert torch.equal(r[0], acc) and torch.equal(r[1], path) and torch.equal(r[2], toks), c.name
        assert int(acc.max()) < c.max_path                    # inside tree_verify's precondition
        if c.expect_accept is not None:
            assert acc.tolist() == c.expect_accept, c.name
            assert [int(path[0, int(acc[0])])] == c.expect_best, c.name
    names = [c.name for c in sc.tree_cases()]
    chain = sc.tree_cases()[names.index("chain of 64, all accepted")]
    assert int(sc.brute_tree(chain)[0][0, 63]) == -1 and int(sc.brute_tree(chain)[2][0]) == chain.max_path - 1
    b63 = sc.tree_cases()[names.index("bit 63 accepted next to a failed chain")]
    assert int(sc.brute_tree(b63)[0][0, 63]) == -(1 << 63) + 1


# ---- slips ---------------------------------------------------------------------------------------

def _rejecting(mutant, cases):
    return [c.name for c in cases if sc.check_sample(c, sc.kernel_model(c, mutant))]


def test_every_sampling_slip_is_rejected_for_its_reason():
    cases = _all_sample_cases() + _tie_cases()
    hit = {m: _rejecting(m, cases) for m in sc.MUTANTS}
    for m, names in hit.items():
        print(f"COUNT slip '{m}' rejected by {len(names)} of {len(cases)} cases")
        assert names, m
    # where each slip must show: sampled rows / a row ending after a 16-byte vector / the split path /
    # planted ties / a pick on the threshold itself / rows with T != 1
    assert all("greedy ties" not in n for n in hit["hash of i + 1"])
    assert any("greedy ties V=4099" in n for n in hit["last V % 8 elements dropped"])
    assert all(int(n.split("V=")[1].split()[0]) % 8 for n in hit["last V % 8 elements dropped"] if "V=" in n)
    assert all("V=" in n and int(n.split("V=")[1].split()[0]) >= 2 * sc.SP_CHUNK or "u=1" in n
               for n in hit["chunk offset not added"])
    assert any("greedy ties" in n for n in hit["ties to the higher index"])
    assert any("top_k = 1" in n for n in hit["v <= thresh skipped"])
    assert all("filtered" in n or "top_k = 1" in n for n in hit["v <= thresh skipped"])
    assert all("greedy ties" not in n and "u=1" not in n for n in hit["temperature not applied"])


def test_topk_slips_are_rejected():
    for mutant, chunk in (("ties to the higher index", 0), ("last V % 8 elements dropped", 0),
                          ("chunk offset not added", sc.TK_CHUNK)):
        hit = 0
        for V in sc.TKL_V + sc.TOPK_V:
            logits, _ = sc.topk_rows(V, torch.bfloat16, chunk_ties=(2047, 2048) if V in sc.TKL_V else ())
            for k in (1, 8):
                v, i = sc.topk_model(logits, k, mutant, chunk)
                rv, ri = sc.topk_ref(logits, k)
                hit += not (torch.equal(i, ri) and torch.equal(v.double(), rv))
                v, i = sc.topk_model(logits, k)                       # the model without a slip is the reference
                assert torch.equal(i, ri) and torch.equal(v.double(), rv), (V, k)
        assert hit, mutant


def test_tree_slips_are_rejected():
    names = {c.name: c for c in sc.tree_cases()}
    for kw, must in ((dict(parent_only=True), "matches under a failed ancestor are rejected"),
                     (dict(tie_high=True), "two accepted leaves of equal depth")):
        differs = [c.name for c in sc.tree_cases()
                   if not all(torch.equal(a, b) for a, b in zip(sc.brute_tree(c, **kw)[2:], sc.brute_tree(c)[2:]))]
        assert must in differs, (kw, differs)
    c = names["chain of 64, node 40 fails, its descendants match their parents"]
    assert int(sc.brute_tree(c, parent_only=True)[2][0]) == 63 and int(sc.brute_tree(c)[2][0]) == 39
    assert int(sc.brute_tree(names["star, two matching leaves"], tie_high=True)[3][0, 1]) == 40
