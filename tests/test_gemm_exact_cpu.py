"""tests/gemm_cases.py judged on the CPU: every case's exactness conditions, the DELTA measurement,
the launch-plan model against hand-worked plans, and — the point of the file — that the comparator
which judges the GPU kernels rejects a model kernel with any one of the listed slips and passes the
model without one."""
import pytest
import torch

import gemm_cases as gc
from dgi import ops


def _small_cases():
    yield "dense 17x256x64", gc.dense(17, 256, 64, 1)
    yield "dense 129x256x512", gc.dense(129, 256, 512, 2)
    yield "dense 200x256x1152", gc.dense(200, 256, 1152, 3)
    yield "probe 200x256x512", gc.probe(200, 256, 512)
    yield "fold 200x256x512", gc.fold_probe(200, 256)
    yield "residual 257x512x256", gc.residual(257, 512, 256, 4)
    yield "residual 100x512x512", gc.residual(100, 512, 512, 5)
    for kind in (3, 4):
        yield f"normed {kind} 257x512x512", gc.normed(257, 512, 512, kind, 6 + kind, ss_ld=16)
        yield f"normed {kind} 200x256x1152", gc.normed(200, 256 * (kind - 2), 1152, kind, 8 + kind, ss_ld=32)
    yield "rope 2/2 257x768x256", gc.normed_rope(257, 2, 2, 256, 12)
    yield "rope 4/2 100x1024x512", gc.normed_rope(100, 4, 2, 512, 13, ss_ld=24)
    for pro in (0, 1, 2):
        yield f"fused pro {pro} epi 0", gc.fused(16, 32, 1024, pro, 0, 20 + pro)
        yield f"fused pro {pro} epi 1", gc.fused(15, 32, 1024, pro, 1, 23 + pro)
        yield f"fused pro {pro} epi 2", gc.fused(16, 768, 1024, pro, 2, 26 + pro, nh=2, nkv=2)
    yield "fused sparse pro 1 epi 0", gc.fused(16, 32, 4096, 1, 0, 29, sparse=True)
    for name, c in gc.swiglu_cpu_cases():
        yield name, c


def test_every_case_meets_its_exactness_conditions():
    n = 0
    for name, c in _small_cases():
        try:
            gc.check(c)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from None
        n += 1
    assert n >= 30


def test_check_rejects_an_inexact_case():
    """The conditions are live: W in ±3 at K = 1152 leaves the bf16 integers, and a row of partials
    that does not add up to K * 4^-j is caught."""
    c = gc.dense(64, 256, 1152, 3)
    c.w64 = c.w64 * 3
    c.y64 = c.xin64 @ c.w64.T
    with pytest.raises(AssertionError):
        gc.check(c)
    with pytest.raises(AssertionError, match="power of four"):
        c = gc.normed(8, 256, 256, 3, 1)
        c.ss[3, 5] *= 3
        gc.check(c)


def test_fp32_gap_is_the_recorded_one():
    worst = 0.0
    for _, c in gc.swiglu_cpu_cases():
        g, u = gc.gate_up(c)
        f32 = ops.silu_mul_ref(torch.cat([g, u], 1).float()).double()
        nz = c.r64 != 0
        worst = max(worst, float(((f32 - c.r64).abs()[nz] / c.r64.abs()[nz]).max()))
    print(f"RATIO fp32-vs-fp64 gap {worst:.3e} recorded {gc.FP32_GAP:.3e} delta {gc.DELTA:.3e}")
    assert 0.95 * gc.FP32_GAP <= worst <= gc.FP32_GAP
    assert gc.DELTA == 16 * gc.FP32_GAP


def test_non_decisive_elements_stay_under_the_cap():
    for name, c in gc.swiglu_cpu_cases():
        share = gc.non_decisive(c.r64) / c.r64.numel()
        print(f"RATIO non-decisive {name} {share:.5f}")
        assert share <= gc.MAX_NON_DECISIVE, name


def test_neighbour_rule_takes_the_nearest_value_and_no_other_far_from_a_tie():
    r = torch.tensor([1.0 + 2.0 ** -9, 3.14159, -100.3, 0.0, 2.0 ** -20 * 1.37], dtype=torch.float64)
    near = gc.to_bf16(r)
    assert not bool(gc.judge(near, r)[0].any())
    up = (near.view(torch.int16) + 1).view(torch.bfloat16)
    assert gc.judge(up, r)[0].tolist() == [True, True, True, True, True]
    # r[0] sits a hair above the midpoint of 1 and 1 + 2^-7: the value below it is out, the tie itself is in both ways
    tie = torch.tensor([1.0 + 2.0 ** -8], dtype=torch.float64)
    for b in (1.0, 1.0 + 2.0 ** -7):
        assert not bool(gc.judge(torch.tensor([b], dtype=torch.bfloat16), tie)[0].any())
    assert gc.non_decisive(tie) == 1 and gc.non_decisive(r) == 0


def test_pp_plan_matches_hand_worked_plans():
    P = 256
    plan = lambda *a: gc.pp_plan(*a, P)                                             # noqa: E731
    one = dict(tiles=1, grid=1, persistent=False, rem=0, splits=0, full=0)
    assert plan(200, 256, 256, False, 0, True) == one                               # 4 K tiles: never split
    assert plan(200, 256, 512, False, 1, False) == one                              # split-K off, no overlap
    assert plan(200, 256, 512, False, 0, True) == dict(tiles=1, grid=256, persistent=True, rem=1, splits=4, full=0)
    assert gc.pieces(512, 4) == [(0, 128), (128, 256), (256, 384), (384, 512)]
    assert gc.pieces(640, 4) == [(0, 128), (128, 256), (256, 384), (384, 640)]      # 5 units: 1, 1, 1, 2
    assert gc.pieces(1152, 4) == [(0, 256), (256, 512), (512, 768), (768, 1152)]    # 9 units: 2, 2, 2, 3
    assert plan(700, 1280, 256, False, 0, True)["grid"] == 15
    assert plan(1271, 3328, 640, False, 0, True) == dict(tiles=65, grid=256, persistent=True, rem=65, splits=3, full=0)
    assert plan(2040, 2816, 512, False, 0, True) == dict(tiles=88, grid=256, persistent=True, rem=88, splits=2, full=0)
    assert plan(4096, 4352, 512, False, 0, True) == dict(tiles=272, grid=256, persistent=True, rem=16, splits=4, full=1)
    assert plan(3072, 2816, 512, False, 0, True) == dict(tiles=132, grid=132, persistent=False, rem=0, splits=0, full=0)
    assert plan(3072, 2816, 512, False, 2, True)["persistent"] is False             # 256 // 132 = 1 piece
    assert plan(4096, 8192, 512, False, 0, True) == dict(tiles=512, grid=256, persistent=True, rem=0, splits=0, full=2)
    assert plan(4096, 8192, 512, False, 0, False)["grid"] == 512
    # SwiGLU: 128 output columns per tile, N = 2 I rows of W
    assert plan(200, 256, 512, True, 0, True)["tiles"] == 1 and plan(700, 2560, 256, True, 0, True)["tiles"] == 30
    # 9 full waves + 1 tile: auto leaves it whole (full >= 8), streamk 2 cuts it
    assert plan(256, 256 * 2305, 512, False, 0, False)["persistent"] is False
    assert plan(256, 256 * 2305, 512, False, 2, False) == dict(tiles=2305, grid=256, persistent=True, rem=1, splits=4,
                                                               full=9)
    # another CU count: the case recomputes its N
    assert gc.n_for(dict(splits=3, full=0), 1271, 3328, 640, 256) == 3328
    n = gc.n_for(dict(splits=3, full=0), 1271, 3328, 640, 304)
    assert n != 3328 and gc.pp_plan(1271, n, 640, False, 0, True, 304)["splits"] == 3


# mutation -> the families (smallest case of each) whose comparator must reject it
def _families():
    return {
        "plain": gc.dense(17, 256, 64, 1),
        "split": gc.dense(200, 256, 512, 31),
        "fold": gc.fold_probe(200, 256),
        "probe": gc.probe(200, 256, 512),
        "swiglu": gc.swiglu(17, 128, 64, 32),
        "res": gc.residual(100, 256, 512, 33),
        "norm": gc.normed(100, 256, 256, 3, 34),
        "normswiglu": gc.normed(100, 512, 256, 4, 35),
        "rope": gc.normed_rope(100, 2, 2, 256, 36),
        "fused0": gc.fused(16, 32, 1024, 1, 0, 37),
        "fused1": gc.fused(16, 32, 1024, 2, 1, 38),
        "fused2": gc.fused(16, 768, 1024, 0, 2, 39, nh=2, nkv=2),
    }


REJECTED_BY = {
    "drop_k": ("plain", "split", "swiglu", "res", "norm", "normswiglu", "rope", "fused0", "fused1", "fused2"),
    "swap_chunks": ("plain", "split", "probe", "swiglu", "res", "norm", "rope", "fused0", "fused2"),
    "truncate": ("swiglu", "normswiglu", "res", "fused1"),
    "round_piece": ("fold",),
    "skip_piece": ("split", "fold", "probe"),
    "row_past_m": ("plain", "swiglu", "res", "norm", "normswiglu", "rope", "fused0", "fused1", "fused2"),
    "ss_fp32": ("res",),
    "short_ss": ("norm", "normswiglu", "rope"),
    "partner32": ("rope", "fused2"),
    "sin_sign": ("rope", "fused2"),
    "swap_gate_up": ("swiglu", "normswiglu", "fused1"),
}
SPLIT = {"split": 4, "fold": 4, "probe": 4}


@pytest.fixture(scope="module")
def families():
    return {k: gc.check(c) for k, c in _families().items()}


def _judged(c):
    """(case as the GPU test judges it, model arguments): fused cases are judged with their bias."""
    if c.kind.startswith("fused"):
        return gc.with_answer(c, c.withbias), dict(bias=True)
    return c, {}


def test_the_unmutated_model_passes(families):
    for fam, c in families.items():
        jc, kw = _judged(c)
        for splits in {1, SPLIT.get(fam, 1)}:
            fails, _ = gc.verdict(jc, **gc.kernel_model(c, None, splits=splits, **kw))
            assert not fails, f"{fam} splits {splits}: {fails}"


@pytest.mark.parametrize("mutation", gc.MUTATIONS)
def test_every_mutation_is_rejected(families, mutation):
    assert set(REJECTED_BY) == set(gc.MUTATIONS)
    for fam in REJECTED_BY[mutation]:
        c = families[fam]
        jc, kw = _judged(c)
        fails, _ = gc.verdict(jc, **gc.kernel_model(c, mutation, splits=SPLIT.get(fam, 1), **kw))
        assert fails, f"{mutation} passed on {fam}"
