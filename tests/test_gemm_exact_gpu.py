"""mfma_gemm, mfma_gemm_norm, mfma_gemm_norm_rope, fused_skinny and decode_proj against inputs whose
answer is known exactly (tests/gemm_cases.py).

Run on an MI355X (``pytest -m gpu``).  Exact families must meet the float64 answer bit for bit, in
every schedule, phase count, split-K policy and launch config; every output goes into a window of a
sentinel buffer and every cell outside the window must still hold the sentinel.  The SwiGLU families
are judged by the neighbour rule and print ``RATIO <family> <kernel> <worst |b - r64| / allowance>``
(``pytest -s``); the ratios are recorded in profiles/gemm_exact/README.md.  Each multi-tile case names
the launch plan it is meant to reach and asserts it for the device's CU count
(tests/test_gemm_exact_cpu.py proves that the comparator rejects a kernel with any single slip).
"""
import types

import pytest
import torch

import gemm_cases as gc
from dgi import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16

ONE_TILE_MS = (1, 15, 16, 17, 127, 128, 129, 255, 256)
ONE_TILE_KS = (64, 128, 192, 256, 384, 512)      # 64-192 and 384: the simple kernel for sched 3; 256: four K tiles
# sched, phases, streamk, overlap
SCHEDULES = [(0, 0, 0, True), (1, 0, 0, True)] + [(3, ph, sk, ov) for ph in (2, 4) for sk in (0, 1, 2)
                                                  for ov in (True, False)]

# name, M, N at 256 CUs, K, the plan reached with streamk 0 and overlap on
PATHS = [
    ("15 tiles, grid no multiple of 8", 700, 1280, 256, dict(tiles=15, grid=15, persistent=False)),
    ("lone tile cut in 4, one unit per piece", 200, 256, 512, dict(tiles=1, persistent=True, rem=1, splits=4, full=0)),
    ("lone tile cut in 4, uneven pieces", 200, 256, 640, dict(tiles=1, persistent=True, rem=1, splits=4, full=0)),
    ("lone tile cut in 4, K 1152", 200, 256, 1152, dict(tiles=1, persistent=True, rem=1, splits=4, full=0)),
    ("3 pieces", 1271, 3328, 640, dict(persistent=True, splits=3, full=0)),
    ("2 pieces", 2040, 2816, 512, dict(persistent=True, splits=2, full=0)),
    ("pieces, then a whole tile per block", 4096, 4352, 512, dict(persistent=True, splits=4, full=1)),
    ("more than half a wave, no split", 3072, 2816, 512, dict(persistent=False, splits=0)),
    ("two whole waves, persistent", 4096, 8192, 512, dict(persistent=True, rem=0, splits=0, full=2)),
]
# phases, streamk, overlap of the multi-tile runs; the first is the one whose plan the case names
PATH_RUNS = [(2, 0, True), (4, 0, True), (2, 0, False), (4, 1, True), (2, 1, False), (4, 2, True)]

NORM_MS = (1, 100, 256, 257)
NORM_KS = (256, 512)
NORM_SS_LD = {256: 8, 512: 32, 1152: 16}

FUSED_MS = (1, 2, 15, 16)
FUSED_R = {0: (32, 8224), 1: (32, 8224), 2: (768, 6144)}          # epi -> rows of W; epi 2: nh / nkv = 2 / 2, 32 / 8
FUSED_HEADS = {768: (2, 2), 6144: (32, 8)}


@pytest.fixture(autouse=True, scope="module")
def _native():
    ops.load_native(required=True)


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count & ~7


def head(c, M):
    """Case c cut to its first M rows."""
    d = types.SimpleNamespace(**c.__dict__)
    d.M = M
    for k in ("x", "ref", "r64"):
        if getattr(c, k) is not None:
            setattr(d, k, getattr(c, k)[:M])
    return d


def wide(x):
    """x as a window of a wider buffer of other values (row stride K + 16)."""
    buf = torch.full((x.shape[0] + 1, x.shape[1] + 16), 3.0, dtype=BF, device=x.device)
    buf[:x.shape[0], 8:8 + x.shape[1]] = x
    return buf[:x.shape[0], 8:8 + x.shape[1]]


def window(c):
    buf = torch.full((c.M + gc.TAIL, c.cols + 2 * gc.PAD), gc.SENT, dtype=BF, device=DEV)
    return buf, buf[:c.M, gc.PAD:gc.PAD + c.cols]


class Tally:
    def __init__(self, family, kernel):
        self.family, self.kernel, self.fails, self.worst, self.n, self.ratio = family, kernel, [], 0.0, 0, False

    def add(self, what, c, buf, **out):
        fails, worst = gc.verdict(c, buf, **out)
        self.fails += [f"{what}: {f}" for f in fails]
        self.worst = max(self.worst, worst)
        self.ratio |= c.ref is None
        self.n += 1

    def done(self):
        if self.ratio:
            print(f"RATIO {self.family} {self.kernel} {self.worst:.4f}")
        assert not self.fails, f"{len(self.fails)} of {self.n} runs failed:\n" + "\n".join(self.fails[:12])
        assert ops.gemm_split_timeouts(reset=True) == 0


def plain_case(M, N, K, epi, seed):
    """mfma_gemm's case: N rows of W (epi 1: N / 2 gate and N / 2 up rows)."""
    return gc.check(gc.swiglu(M, N // 2, K, seed, DEV) if epi else gc.dense(M, N, K, seed, DEV))


def run_plain(c, epi, x, sched=3, phases=0, streamk=0, overlap=True):
    buf, win = window(c)
    ops.mfma_gemm(x, c.w, epi, out=win, sched=sched, streamk=streamk, phases=phases, overlap=overlap)
    return buf


# ---------------------------------------------------------------------------------------------
# mfma_gemm, epi 0 and 1
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("epi", [0, 1])
@pytest.mark.parametrize("K", ONE_TILE_KS)
def test_one_tile_every_schedule(K, epi):
    """One 256 x 256 tile (epi 1: 256 rows of W, 128 columns) at every row-count edge, through the
    simple kernel (sched 0 / 1, and sched 3 where K does not fit the ping-pong kernel), the ping-pong
    kernel in 2 and 4 phases and, at K = 512, its four-piece split (streamk 0 / 2)."""
    big = plain_case(256, 256, K, epi, 100 + K + epi)
    t = Tally("swiglu" if epi else "plain", f"mfma_gemm K={K}")
    P = cu_count()
    assert gc.pp_plan(256, 256, K, bool(epi), 0, True, P)["splits"] == (4 if K == 512 else 0)
    for M in ONE_TILE_MS:
        c = head(big, M)
        for i, (sched, ph, sk, ov) in enumerate(SCHEDULES):
            x = wide(c.x) if (i + M) & 1 else c.x
            t.add(f"M {M} sched {sched} phases {ph} streamk {sk} overlap {ov}", c, run_plain(c, epi, x, sched, ph, sk, ov))
        t.add(f"M {M} defaults, contiguous", c, run_plain(c, epi, c.x))
        t.add(f"M {M} defaults, row slice", c, run_plain(c, epi, wide(c.x)))
    t.done()


@pytest.mark.parametrize("epi", [0, 1])
@pytest.mark.parametrize("path", PATHS, ids=[p[0] for p in PATHS])
def test_multi_tile_paths(path, epi):
    """Each work decomposition of launch_pp at the smallest shape that reaches it (the plan is
    asserted for this device's CU count; N is recomputed from it on another device).  Every launch
    runs twice: the second must be exact too (the split counters returned to zero)."""
    name, M, N, K, want = path
    P = cu_count()
    N = gc.n_for(want, M, N, K, P)
    plan = gc.pp_plan(M, N, K, bool(epi), 0, True, P)
    assert all(plan[k] == v for k, v in want.items()), (name, plan)
    if name.startswith("more than half"):
        assert plan["tiles"] > P // 2 and plan["grid"] == plan["tiles"]
    if name.startswith("two whole waves"):
        assert gc.pp_plan(M, N, K, bool(epi), 0, False, P) == dict(tiles=2 * P, grid=2 * P, persistent=False, rem=0,
                                                                  splits=0, full=0)
    c = plain_case(M, N, K, epi, 200 + M % 97 + K + epi)
    t = Tally("swiglu" if epi else "plain", f"mfma_gemm {name}")
    for i, (ph, sk, ov) in enumerate(PATH_RUNS):
        x = wide(c.x) if i == 1 else c.x
        for rep in range(2):
            t.add(f"phases {ph} streamk {sk} overlap {ov} run {rep} plan {gc.pp_plan(M, N, K, bool(epi), sk, ov, P)}", c,
                  run_plain(c, epi, x, 3, ph, sk, ov))
        assert ops.gemm_split_timeouts(reset=True) == 0
    t.done()


def test_fold_keeps_every_bit_of_a_piece():
    """Four pieces whose fp32 partials carry 16 significant bits (gemm_cases.fold_probe): a fold that
    rounds a slab, or skips one, misses the integer total."""
    c = gc.check(gc.fold_probe(200, 256, DEV))
    assert gc.pp_plan(200, 256, 512, False, 0, True, cu_count())["splits"] == 4
    t = Tally("fold", "mfma_gemm")
    for ph in (2, 4):
        for sk in (0, 1, 2):
            for rep in range(2):
                t.add(f"phases {ph} streamk {sk} run {rep}", c, run_plain(c, 0, c.x, 3, ph, sk))
    t.done()


def test_address_probes():
    """One-hot rows: Y[m, n] must be W[n, k_m], at a single tile, a four-piece split and two
    persistent waves; a mismatch names the (n, k) that was read instead."""
    P = cu_count()
    t = Tally("probe", "mfma_gemm")
    n2 = gc.n_for(dict(persistent=True, rem=0, full=2), 4096, 8192, 512, P)
    for M, N, K, want in ((200, 256, 256, dict(persistent=False)), (200, 256, 512, dict(splits=4)),
                          (4096, n2, 512, dict(persistent=True, full=2))):
        plan = gc.pp_plan(M, N, K, False, 0, True, P)
        assert all(plan[k] == v for k, v in want.items())
        c = gc.check(gc.probe(M, N, K, DEV))
        for sched, ph in ((1, 0), (3, 2), (3, 4)):
            for rep in range(2):
                t.add(f"{M}x{N}x{K} sched {sched} phases {ph} run {rep}", c, run_plain(c, 0, c.x, sched, ph))
    t.done()


# ---------------------------------------------------------------------------------------------
# mfma_gemm_norm (kinds 2 - 4) and mfma_gemm_norm_rope
# ---------------------------------------------------------------------------------------------

def _norm_shapes():
    return [(M, 512, K) for K in NORM_KS for M in NORM_MS] + [(200, 256, 1152)]


def test_residual_epilogue():
    """Kind 2: Y + X W^T in place (ties between bf16 neighbours included) and the row statistics of
    the STORED values, bit for bit; cells of ss the kernel does not own keep their fill."""
    t = Tally("residual", "mfma_gemm_norm kind 2")
    for M, N, K in _norm_shapes():
        c = gc.check(gc.residual(M, N, K, 300 + M + K, DEV))
        nt = N // 256
        for ph in (2, 4):
            for rep in range(2):
                buf, win = window(c)
                win.copy_(c.y_old)
                ss = torch.full((M + 1, nt + 1), -1.0, device=DEV)
                ops.mfma_gemm_norm(c.x, c.w, ops.NORM_RES, ss, 0.0, out=win, phases=ph)
                t.add(f"{M}x{N}x{K} phases {ph} run {rep}", c, buf, ss=ss[:M, :nt].contiguous())
                assert bool((ss[M] == -1).all()) and bool((ss[:, nt] == -1).all()), "ss written outside [M, N / 256]"
    t.done()


@pytest.mark.parametrize("kind", [3, 4])
def test_normalised_epilogues(kind):
    """Kinds 3 / 4 with rstd = 2^(m % 3) from partials spread over every column of ss."""
    t = Tally("norm" if kind == 3 else "normswiglu", f"mfma_gemm_norm kind {kind}")
    for M, N, K in _norm_shapes():
        c = gc.check(gc.normed(M, N, K, kind, 400 + M + K + kind, DEV, ss_ld=NORM_SS_LD[K]))
        for ph in (2, 4):
            for rep in range(2):
                buf, win = window(c)
                ss = c.ss.clone()
                ops.mfma_gemm_norm(wide(c.x) if rep else c.x, c.w, kind, ss, 0.0, out=win, phases=ph)
                t.add(f"{M}x{N}x{K} phases {ph} run {rep}", c, buf)
                assert torch.equal(ss, c.ss), "ss changed"
    t.done()


@pytest.mark.parametrize("nh,nkv", [(2, 2), (4, 2)])
def test_normalised_rope_epilogue(nh, nkv):
    """EPI 5 with quarter-turn tables: rotated q in Y, rotated k and raw v in the paged caches, the
    k / v columns of Y, the cache rows of slot -1 and every other cache cell untouched."""
    t = Tally("rope", f"mfma_gemm_norm_rope {nh}/{nkv}")
    for K in NORM_KS:
        for M in NORM_MS:
            c = gc.check(gc.normed_rope(M, nh, nkv, K, 500 + M + K + nh, DEV, ss_ld=NORM_SS_LD[K]))
            for ph in (2, 4):
                buf, win = window(c)
                kc, vc = (torch.full((gc.NB, nkv, gc.BS, 128), gc.SENT, dtype=BF, device=DEV) for _ in range(2))
                ops.mfma_gemm_norm_rope(c.x, c.w, c.ss.clone(), 0.0, c.pos, c.table, c.slots, kc, vc, nh, nkv, out=win,
                                        phases=ph)
                t.add(f"M {M} K {K} phases {ph}", c, buf, kc=kc, vc=vc)
    t.done()


# ---------------------------------------------------------------------------------------------
# fused_skinny and decode_proj
# ---------------------------------------------------------------------------------------------

def _fused_call(c, cfg, bias, K=None):
    buf, win = window(c)
    nkv = max(c.nkv, 1)
    kc, vc = (torch.full((gc.NB, nkv, gc.BS, 128), gc.SENT, dtype=BF, device=DEV) for _ in range(2))
    ro = torch.full_like(c.x, gc.SENT) if c.pro == 2 else None
    epi2 = c.epi == 2
    ops.fused_skinny(win, c.x, c.res, ro, c.gamma, 0.0, c.w, c.bias if bias else None, c.pro, c.epi,
                     c.pos if epi2 else None, c.table if epi2 else None, c.slots if epi2 else None,
                     kc if epi2 else None, vc if epi2 else None, c.nh, c.nkv, cfg=cfg)
    return buf, dict(kc=kc, vc=vc, res_out=ro) if epi2 else dict(res_out=ro)


def fused_k(cfg):
    """The smallest K (1024, 2048, 4096) config cfg accepts: its K-divisibility code is -7."""
    for K in (1024, 2048, 4096):
        c = gc.fused(1, 32, K, 0, 0, 1, DEV, sparse=K > 1024)
        try:
            _fused_call(c, cfg, False)
            return K
        except RuntimeError as e:
            if "code -7" not in str(e):
                raise
    return None


@pytest.mark.parametrize("epi", [0, 1, 2])
@pytest.mark.parametrize("pro", [0, 1, 2])
def test_fused_skinny_every_config(pro, epi):
    """Every launch config at the smallest K it accepts, the smallest R, the persistent configs'
    multi-tile ring with a one-tile last workgroup (R = 8224) and both qkv widths, with and without
    bias, at the row counts around the 16-row MFMA tile.  None is skipped."""
    ks = {cfg: fused_k(cfg) for cfg in sorted(ops.FUSED_CFGS)}
    assert all(ks.values()), f"a config accepts no K up to 4096: {ks}"
    t = Tally(f"fused{epi}", f"fused_skinny pro {pro} epi {epi}")
    ran = 0
    for K in sorted(set(ks.values())):
        for R in FUSED_R[epi]:
            nh, nkv = FUSED_HEADS.get(R, (0, 0)) if epi == 2 else (0, 0)
            for M in FUSED_MS:
                # sparse rows need 4 rows to cover every k: below that K = 4096 keeps dense ±1 rows at pro 0 only
                c = gc.check(gc.fused(M, R, K, pro, epi, 600 + 16 * pro + epi + M + R % 89, DEV, nh=nh, nkv=nkv,
                                      sparse=K > 1024 and M >= 4))
                for cfg in sorted(ops.FUSED_CFGS):
                    if ks[cfg] != K:
                        continue
                    for bias in (False, True):
                        buf, out = _fused_call(c, cfg, bias)
                        t.add(f"cfg {cfg} K {K} R {R} M {M} bias {bias}", gc.with_answer(c, c.withbias if bias else c.nobias),
                              buf, **out)
                        ran += 1
    assert ran == len(ops.FUSED_CFGS) * len(FUSED_R[epi]) * len(FUSED_MS) * 2
    t.done()


def test_decode_proj():
    """The batch-1 o-proj through the persistent fused GEMV: dense ±1 and the address probe."""
    for c in (gc.check(gc.dense(1, 256, 1024, 700, DEV)), gc.check(gc.probe(1, 256, 1024, DEV))):
        assert ops.fused_decode_ok(1, 1024, "qkv")
        y = ops.decode_proj(c.x, c.w)
        assert torch.equal(y, c.ref), (y, c.ref)
