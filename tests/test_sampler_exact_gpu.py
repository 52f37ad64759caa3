"""sampler.hip and tree.hip against inputs whose answer is known exactly (tests/sampler_cases.py).

Run on an MI355X (``pytest -m gpu``).  ``sample`` picks are held to the float64 Gumbel-max scores
(``pick_ok``), thresholds of rows with a known kept set to the reference bit for bit, ``topk`` /
``topk_logprobs`` to a stable sort of float64 values, ``tree_mask`` / ``tree_verify`` to a
brute-force walk of every root-to-leaf path.  tests/test_sampler_exact_cpu.py shows that the
comparators reject one-slip kernel models.  Each test prints ``RATIO`` / ``COUNT`` lines
(``pytest -s``); they are recorded in profiles/sampler_exact/README.md.
"""
import pytest
import torch

import sampler_cases as sc
from dgi import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True, scope="module")
def _native():
    ops.load_native(required=True)


def _run_sample(c, view_names=("contiguous",)):
    """Failures of ``ops.sample`` on ``c`` through the named views, and the non-decisive row count."""
    bad = []
    kw = c.kwargs(DEV)
    for name, lg in sc.views(c.logits.to(DEV)):
        if name in view_names:
            picks = ops.sample(lg, **kw)
            bad += [f"[{name}] {m}" for m in sc.check_sample(c, picks)]
            if c.filt:                                   # the set the kernel sampled from is the reference's
                th = ops.topkp_threshold(lg, kw["temperature"], kw["top_k"], kw["top_p"]).cpu().tolist()
                bad += [f"[{name}] {c.name} row {b}: threshold {t} != {r}"
                        for b, (t, r) in enumerate(zip(th, c.thresholds())) if t != r]
    return bad, c.non_decisive()


ALL_VIEWS = ("contiguous", "odd stride", "stride % 8 == 0, aligned", "stride % 8 == 0, base + 1")


@pytest.mark.parametrize("filt", [False, True], ids=["plain", "filtered"])
@pytest.mark.parametrize("dtype", sc.DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("V", sc.ONE_WG_V + sc.SPLIT_V)
def test_sample_picks(V, dtype, filt):
    c = next(x for x in sc.sample_cases()
             if x.logits.shape == (8, V) and x.logits.dtype == dtype and x.filt == filt)
    bad, nd = _run_sample(c, ALL_VIEWS)
    print(f"COUNT sample {c.name}: non-decisive rows {nd} of {c.sampled_rows()}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("filt", [False, True], ids=["plain", "filtered"])
@pytest.mark.parametrize("dtype", sc.DTYPES, ids=["bf16", "fp32"])
def test_sample_picks_33_rows_take_one_workgroup_per_row(dtype, filt):
    c = next(x for x in sc.sample_cases()
             if x.logits.shape == (33, 16384) and x.logits.dtype == dtype and x.filt == filt)
    bad, nd = _run_sample(c)
    print(f"COUNT sample {c.name}: non-decisive rows {nd} of {c.sampled_rows()}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("V", sc.BIG_V)
def test_sample_picks_full_vocabularies(V):
    c = next(x for x in sc.sample_cases() if x.logits.shape[1] == V)
    bad, nd = _run_sample(c)
    print(f"COUNT sample {c.name}: non-decisive rows {nd} of {c.sampled_rows()}")
    assert not bad, "\n".join(bad)


def test_sample_top_k_1_picks_the_threshold_element():
    c = sc.k1_case()
    bad, nd = _run_sample(c, ALL_VIEWS)
    print(f"COUNT sample {c.name}: non-decisive rows {nd} of {c.sampled_rows()}, {len(bad)} failures")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("dtype", sc.DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("V", [1023, 4099, 8200, 16385, 24571])
def test_greedy_ties_go_to_the_lowest_index(V, dtype):
    c = sc.greedy_tie_case(V, dtype)
    bad, _ = _run_sample(c, ALL_VIEWS)
    print(f"COUNT {c.name}: {c.logits.shape[0]} rows with planted ties x 4 views, {len(bad)} failures")
    assert not bad, "\n".join(bad)
    lg = c.logits.to(DEV)
    assert not sc.check_sample(c, ops.sample(lg))                       # no temperature at all
    c40 = sc.SampleCase(c.name + " x4", c.logits.repeat(4, 1), c.temps.repeat(4), c.seeds.repeat(4), 0)
    assert not sc.check_sample(c40, ops.sample(lg.repeat(4, 1)))       # > 32 rows: one workgroup per row


def test_sample_u1_pairs_do_not_pick_the_planted_id():
    """(seed, id) pairs whose 24-bit uniform rounded to 1.0 (noise +inf): with logit -30 at the id
    the pick must be the float64 winner, in particular not that id."""
    for c in sc.u1_cases():
        picks = ops.sample(c.logits.to(DEV), **c.kwargs(DEV))
        planted = [p == sc.U1_PAIRS[b % 8][1] for b, p in enumerate(picks.cpu().tolist())]
        print(f"COUNT {c.name}: rows that picked the planted id {sum(planted)} of {len(planted)}; "
              f"non-decisive rows {c.non_decisive()}")
        bad = sc.check_sample(c, picks)
        assert not any(planted) and not bad, "\n".join(bad)


# ---- thresholds -------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", sc.DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("V", sc.THRESH_V)
def test_threshold_of_known_kept_sets_is_exact(V, dtype):
    c = sc.thresh_case(V, dtype)
    bad = []
    for vname, lg in sc.views(c.logits.to(DEV)):
        th = ops.topkp_threshold(lg, c.temps.to(DEV), c.top_k.to(DEV), c.top_p.to(DEV)).cpu().tolist()
        bad += [f"[{vname}] {name}: {t} != {r.thresh} (gap {r.gap:.2e})"
                for name, t, r in zip(c.rows, th, c.ref) if t != r.thresh]
    print(f"COUNT thresholds {c.name}: {len(c.rows)} rows x 4 views, {len(bad)} differ")
    assert not bad, "\n".join(bad)


def test_threshold_of_fp32_values_inside_one_search_interval_keeps_a_superset():
    lg, T, k, p, ref, rng = sc.superset_case()
    th = float(ops.topkp_threshold(lg.to(DEV), T.to(DEV), k.to(DEV), p.to(DEV))[0])
    print(f"RATIO superset threshold (ref - got) / (range / 16^6) {(ref - th) / (rng * sc.SEARCH_WIDTH):.4f}")
    assert th <= ref and th >= ref - rng * sc.SEARCH_WIDTH
    assert bool(((lg[0] >= th) | ~(lg[0] >= ref)).all())                # kept is a superset of the reference's


# ---- top-k ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", sc.DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("V", sc.TOPK_V)
def test_topk_is_the_stable_sort(V, dtype):
    logits, names = sc.topk_rows(V, dtype)
    bad = []
    for vname, lg in sc.views(logits.to(DEV)):
        for k in sc.TOPK_K:
            v, i = ops.topk(lg, k)
            rv, ri = sc.topk_ref(logits, k)
            for b, name in enumerate(names):
                if not (torch.equal(i[b].cpu(), ri[b]) and torch.equal(v[b].cpu().double(), rv[b])):
                    bad.append(f"[{vname}] k={k} {name}: {i[b].tolist()} != {ri[b].tolist()}")
    print(f"COUNT topk V={V}: {len(bad)} rows differ")
    assert not bad, "\n".join(bad[:20])
    assert ops.topk(logits[2:3].to(DEV), 8)[1].tolist() == [list(range(8))]          # the constant row


def test_topk_refuses_k_above_v():
    lg = torch.randn(2, 5, device=DEV)
    wide = torch.randn(2, 40, device=DEV)
    refused = 0
    for f in (ops.topk, ops.topk_logprobs):
        for x, k in ((lg, 6), (lg.bfloat16(), 8), (lg, 0), (wide, 17), (wide.bfloat16(), 17)):
            with pytest.raises(ValueError):
                f(x, k)
            refused += 1
    assert ops.topk(lg, 5)[1].shape == (2, 5) and ops.topk(wide, 16)[1].shape == (2, 16)
    print(f"COUNT topk / topk_logprobs calls with k outside 1..min(16, V) refused {refused} of 10")


@pytest.mark.parametrize("V", sc.TKL_V)
def test_topk_logprobs_match_float64(V):
    logits, names = sc.topk_rows(V, torch.bfloat16, chunk_ties=(2047, 2048))
    lp = sc.logprobs64(logits)
    bad, worst = [], 0.0
    # the last view starts 8 bytes into a 16-byte line (offset 4 elements): the wrapper must not
    # hand it to the 16-byte loads of the fused kernels
    lgd = logits.to(DEV)
    B = lgd.shape[0]
    S8 = (V + 15) // 8 * 8
    off4 = torch.zeros(B * S8 + 8, dtype=lgd.dtype, device=DEV).as_strided((B, V), (S8, 1), 4)
    off4.copy_(lgd)
    for vname, lg in list(sc.views(lgd)) + [("stride % 8 == 0, base + 4", off4)]:
        for k in sc.TKL_K:
            v, i = ops.topk_logprobs(lg, k)
            _, ri = sc.topk_ref(logits, k)
            want = lp.gather(1, ri)
            tol = 2e-5 + 1e-5 * want.abs()
            err = (v.cpu().double() - want).abs()
            err = torch.where(v.cpu().double() == want, torch.zeros_like(err), err)       # -inf == -inf
            for b, name in enumerate(names):
                if not torch.equal(i[b].cpu(), ri[b]):
                    bad.append(f"[{vname}] k={k} {name}: indices {i[b].tolist()} != {ri[b].tolist()}")
                elif not bool((err[b] <= tol[b]).all()):
                    bad.append(f"[{vname}] k={k} {name}: log-probs off by {float(err[b].max()):.3e}")
            fin = torch.isfinite(tol)
            if bool(fin.any()):
                worst = max(worst, float((err[fin] / tol[fin]).max()))
    print(f"RATIO topk_logprobs V={V} {worst:.4f}")
    assert not bad, "\n".join(bad[:20])


# ---- draft trees ------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(len(sc.tree_cases())), ids=[c.name for c in sc.tree_cases()])
def test_tree_mask_and_verify(i):
    c = sc.tree_cases()[i]
    anc, depth, acc, path, toks = sc.brute_tree(c)
    a, d = ops.tree_mask(c.parent.to(DEV))
    assert torch.equal(a.cpu(), anc) and torch.equal(d.cpu(), depth)
    r = ops.tree_verify(c.parent.to(DEV), c.draft.to(DEV), c.target.to(DEV), a, d, c.max_path)
    rr = ops.tree_verify_ref(c.parent, c.draft, c.target, anc, depth, c.max_path)
    for name, got, want, ref in zip(("accept_len", "path", "tokens"), r, (acc, path, toks), rr):
        assert torch.equal(got.cpu(), want), (c.name, name, got.cpu().tolist(), want.tolist())
        assert torch.equal(ref, want), (c.name, name)
    print(f"COUNT tree {c.name}: accept lengths {acc.tolist()} of max_path {c.max_path}")
