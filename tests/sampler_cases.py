"""Inputs with exactly known answers for sampler.hip and tree.hip, and their float64 references.

Imported by tests/test_sampler_exact_cpu.py (the references and comparators test themselves, no
GPU) and tests/test_sampler_exact_gpu.py (the HIP kernels).  Four groups:

* **sampled picks** (``ops.sample``).  ``noisy64`` recomputes the Gumbel-max scores in float64
  from the integer hash of ``ops._hash32``: the uniform is an exact dyadic, and
  ``logits / T - log(-log(u))`` is evaluated in float64.  A kernel returns only an index, so
  ``pick_ok`` accepts a pick iff it lies inside the top-k / top-p set and its float64 score is
  within ``DELTA`` of the best score of that set.  ``DELTA`` is not taken from any kernel: it is
  16 x ``FP32_GAP``, the largest ``|noisy_fp32 - noisy64|`` over the committed cases, where
  ``noisy_fp32`` is the CPU path of ``ops.sample`` (fp32, precise ``log``).  The factor covers the
  kernel's ``__logf`` (hardware log2 times ln 2, applied twice, "about 1 ulp") and its
  ``v * (1 / T)``.  A row is *decisive* when one index only passes; at most 1 % of the rows of
  a case may be non-decisive under ``noisy64`` alone (P(top-two gap < DELTA) ~ DELTA), which the
  CPU test asserts for the committed seeds.  Greedy rows (T <= 1e-5) have no noise: the pick is
  the lowest index of the float maximum.
* **thresholds** (``ops.topkp_threshold``).  ``threshold64`` evaluates the keep rule of
  ``topkp_threshold`` per distinct value in float64 and reports how far the mass condition is
  from flipping at the two values next to the cut.  Every committed row has a relative gap of
  at least 1e-3 there (``mid_p`` puts ``top_p`` half-way between two cumulative masses), the
  counts are integers, and the distinct values next to a cut lie further apart than 4 x the
  kernel's final search interval (range / 16^6): so the kernel's threshold, an element value, must
  equal the reference's bit for bit.  With ``top_p = 1`` the mass condition is ``mass_gt(v) <=
  Z_k`` over a subset of the same non-negative terms, true in any summation order, so no gap is
  asked there.  ``superset_case`` is the documented fp32 exception: values closer than
  range / 16^6 at the cut.
* **top-k** (``ops.topk``, ``ops.topk_logprobs``): float64 ``log_softmax`` and a stable sort by
  (-value, index).
* **draft trees** (``ops.tree_mask``, ``ops.tree_verify``): seeded random and hand-made parent
  arrays; ``brute_tree`` walks every root-to-leaf path and is independent of
  ``ops.tree_mask_ref`` / ``ops.tree_verify_ref``.

``kernel_model`` is an fp32 CPU model of the sampling kernels with one switchable slip each
(``mutate=``); the CPU test runs every slip through the comparators to show that they notice.
"""
from __future__ import annotations

import math
import random
from dataclasses import dataclass, field
from typing import Optional

import torch

from dgi import ops

_M32 = 0xFFFFFFFF
NEG_INF = float("-inf")

# max |noisy_fp32 - noisy64| over every sampled case below: 1.610e-6 as measured by
# test_sampler_exact_cpu.py::test_fp32_gap_is_the_recorded_one, which fails if the measurement
# leaves [0.95, 1] x this figure (1.610e-6 rounded up in the third digit)
FP32_GAP = 1.62e-6
DELTA = 16 * FP32_GAP
MAX_NON_DECISIVE = 0.01            # share of a case's sampled rows
MIN_GAP = 1e-3                     # relative distance of the mass condition from flipping
SEARCH_WIDTH = 16.0 ** -6          # final interval of the kernel's threshold search / row range

SP_CHUNK = 8192                    # sampler.hip: logits per workgroup of the split path
TK_CHUNK = 2048                    # sampler.hip: logits per stage-1 workgroup of topk_logprobs

# (seed, token id) whose 24-bit uniform rounded to 1.0 at step 0 before the 23-bit draw
U1_PAIRS = [(148, 114155), (213, 95764), (433, 107696), (460, 123772), (529, 105908), (562, 98187),
            (670, 101259), (698, 126125)]
U1_V = 128256


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------
# sampled picks
# ---------------------------------------------------------------------------------------------

def hash_bits(seeds: torch.Tensor, step: int, V: int, id_shift: int = 0) -> torch.Tensor:
    """h[b, i] = hash32(rowseed_b ^ hash32(i + 0x9e3779b9)) as sampler.hip computes it (int64
    holding uint32 values).  ``id_shift``: the slip "hash of i + 1"."""
    sd = seeds.long().cpu()
    row = ((sd * 2654435761) & _M32) ^ ((step * 40503) & _M32)
    ids = ops._hash32((torch.arange(V, dtype=torch.long) + id_shift + 0x9E3779B9) & _M32)
    return ops._hash32(row[:, None] ^ ids[None, :])


def uniform64(seeds: torch.Tensor, step: int, V: int) -> torch.Tensor:
    """The uniforms as exact dyadics in float64: (top 23 hash bits + 1/2) / 2^23."""
    return ((hash_bits(seeds, step, V) >> 9).double() + 0.5) / 8388608.0


def noisy64(logits: torch.Tensor, temps: torch.Tensor, seeds: torch.Tensor, step: int) -> torch.Tensor:
    """float64 Gumbel-max scores [B, V]; greedy rows (T <= 1e-5) keep their plain logits."""
    lf = logits.detach().cpu().double()
    t = temps.detach().cpu().float().double()
    u = uniform64(seeds, step, lf.shape[1])
    noisy = lf / t.clamp(min=1e-5)[:, None] - torch.log(-torch.log(u))
    return torch.where((t <= 1e-5)[:, None], lf, noisy)


def noisy32(logits: torch.Tensor, temps: torch.Tensor, seeds: torch.Tensor, step: int) -> torch.Tensor:
    """The scores of the CPU path of ``ops.sample`` (fp32, precise log), for measuring FP32_GAP."""
    lf = logits.detach().cpu().float()
    t = temps.detach().cpu().float().clamp(min=1e-5)
    return lf / t[:, None] - torch.log(-torch.log(ops.gumbel_uniform(seeds, step, lf.shape[1], lf.shape[0])))


def candidates(noisy_row: torch.Tensor, logits_row: torch.Tensor, thresh: float, delta: float) -> torch.Tensor:
    """Indices a correct sampler may return for one row: inside {logit >= thresh} and within
    ``delta`` of the best float64 score of that set."""
    inside = logits_row.double() >= thresh
    best = noisy_row[inside].max()
    return (inside & (noisy_row >= best - delta)).nonzero().flatten()


def pick_ok(pick: int, noisy_row: torch.Tensor, thresh: float, delta: float, logits_row: torch.Tensor) -> bool:
    """True iff ``pick`` is inside the threshold set and ``noisy_row[pick] >= max over the set -
    delta``.  On a decisive row exactly one index passes, so the pick must be that index."""
    if not 0 <= pick < noisy_row.numel():
        return False
    return bool((candidates(noisy_row, logits_row, thresh, delta) == pick).any())


@dataclass
class SampleCase:
    name: str
    logits: torch.Tensor                  # [B, V], bf16 or fp32, CPU
    temps: torch.Tensor                   # fp32 [B]; 0 = greedy
    seeds: torch.Tensor                   # int64 [B]
    step: int
    top_k: Optional[torch.Tensor] = None  # int64 [B], with top_p: the filtered call
    top_p: Optional[torch.Tensor] = None
    _ref: dict = field(default_factory=dict, repr=False)

    @property
    def filt(self) -> bool:
        return self.top_k is not None

    def kwargs(self, dev="cpu") -> dict:
        kw = dict(temperature=self.temps.to(dev), seeds=self.seeds.to(dev), step=self.step)
        if self.filt:
            kw.update(top_k=self.top_k.to(dev), top_p=self.top_p.to(dev))
        return kw

    def thresh_refs(self) -> list:
        """``threshold64`` of every row of a filtered case."""
        if "tref" not in self._ref:
            self._ref["tref"] = [threshold64(self.logits[b], float(self.temps[b]), int(self.top_k[b]),
                                             float(self.top_p[b])) for b in range(self.logits.shape[0])]
        return self._ref["tref"]

    def thresholds(self) -> list:
        """float64 reference threshold per row (-inf where nothing is cut)."""
        if not self.filt:
            return [NEG_INF] * self.logits.shape[0]
        return [t.thresh for t in self.thresh_refs()]

    def noisy(self) -> torch.Tensor:
        if "noisy" not in self._ref:
            self._ref["noisy"] = noisy64(self.logits, self.temps, self.seeds, self.step)
        return self._ref["noisy"]

    def allowed(self, delta: float = DELTA) -> list:
        """Per row the tensor of acceptable picks: greedy rows the lowest index of the float
        maximum, sampled rows ``candidates``."""
        key = ("allowed", delta)
        if key not in self._ref:
            th, nz, out = self.thresholds(), self.noisy(), []
            for b in range(self.logits.shape[0]):
                row = self.logits[b].double()
                if float(self.temps[b]) <= 1e-5:
                    out.append((row == row.max()).nonzero().flatten()[:1])
                else:
                    out.append(candidates(nz[b], row, th[b], delta))
            self._ref[key] = out
        return self._ref[key]

    def non_decisive(self, delta: float = DELTA) -> int:
        return sum(1 for a in self.allowed(delta) if a.numel() != 1)

    def sampled_rows(self) -> int:
        return int((self.temps > 1e-5).sum())


def check_sample(c: SampleCase, picks: torch.Tensor, delta: float = DELTA) -> list:
    """Failure messages (empty: every row's pick is acceptable)."""
    picks = picks.detach().cpu().tolist()
    bad = []
    for b, (p, ok) in enumerate(zip(picks, c.allowed(delta))):
        if p not in ok.tolist():
            kind = "greedy" if float(c.temps[b]) <= 1e-5 else "sampled"
            bad.append(f"{c.name} row {b} ({kind}): picked {p}, acceptable {ok.tolist()[:4]}")
    return bad


def _filter_for_rows(logits, temps, seed):
    """Per-row (top_k, top_p) cycling through k only / k then p / p only / no filter, ``top_p``
    placed by ``mid_p`` so that the kept set is known exactly."""
    B, V = logits.shape
    ks, ps = [], []
    for b in range(B):
        T = float(temps[b])
        kind = (b + seed) % 4                     # none / k only / k then p / p only
        k = min((0, 5, 50, 0)[kind], max(1, V - 1))
        ks.append(k)
        if kind < 2:
            ps.append(1.0)
        elif T <= 1e-5:
            ps.append(0.9)                        # a greedy row ignores its filter
        else:
            ps.append(mid_p(logits[b], T, k, 3 if kind == 2 else 20))
    return torch.tensor(ks, dtype=torch.long), torch.tensor(ps, dtype=torch.float32)


def sample_case(V: int, dtype, filt: bool, B: int = 8, seed: int = 0, step: int = 5) -> SampleCase:
    """N(0, 2) rows, temperatures in [0.5, 1.5] with every third row greedy."""
    g = _gen(1000 * seed + V % 997 + (7 if filt else 0) + (13 if dtype == torch.float32 else 0))
    logits = (torch.randn(B, V, generator=g) * 2).to(dtype)
    temps = torch.rand(B, generator=g) + 0.5
    temps[1::3] = 0.0
    seeds = torch.arange(B, dtype=torch.long) * 7 + 1 + seed
    c = SampleCase(f"V={V} B={B} {'bf16' if dtype == torch.bfloat16 else 'fp32'}{' filtered' if filt else ''}",
                   logits, temps, seeds, step)
    if filt:
        c.top_k, c.top_p = _filter_for_rows(logits, temps, seed)
    return c


ONE_WG_V = [1, 7, 8, 1023, 4099, 8200]            # one workgroup per row (V < 2 * SP_CHUNK)
SPLIT_V = [16384, 16385, 24571]                   # split path; 16385: a last chunk of one element
BIG_V = [128256, 151936]                          # once each (bf16, filtered and unfiltered rows mixed)
DTYPES = [torch.bfloat16, torch.float32]

_CACHE: dict = {}


def cached(key, make):
    """Cases and their references are computed once per process and never modified."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def sample_cases() -> list:
    def make():
        cs = [sample_case(V, dt, f) for V in ONE_WG_V + SPLIT_V for dt in DTYPES for f in (False, True)]
        cs += [sample_case(16384, dt, f, B=33) for dt in DTYPES for f in (False, True)]      # B > 32: unsplit
        cs += [sample_case(V, torch.bfloat16, True) for V in BIG_V]
        return cs
    return cached("sample", make)


def k1_case() -> SampleCase:
    """top_k = 1 on every row: the kept set is the maximum alone, so the pick sits on the
    threshold itself (a sampler skipping ``v <= thresh`` has nothing left to pick)."""
    def make():
        c = sample_case(4099, torch.float32, False, seed=3)
        c.name = "top_k = 1 " + c.name
        c.top_k = torch.ones(c.logits.shape[0], dtype=torch.long)
        c.top_p = torch.ones(c.logits.shape[0])
        return c
    return cached("k1", make)


def u1_cases() -> list:
    """The eight (seed, id) pairs at step 0: N(0, 2) rows at V = 128256, T = 1, logit -30 at the
    id.  8 fp32 rows (split path) and the same rows five times over in bf16 (40 rows: one
    workgroup per row)."""
    def make():
        g = _gen(148)
        logits = torch.randn(len(U1_PAIRS), U1_V, generator=g) * 2
        seeds = torch.tensor([s for s, _ in U1_PAIRS], dtype=torch.long)
        for b, (_, i) in enumerate(U1_PAIRS):
            logits[b, i] = -30.0
        one = torch.ones(len(U1_PAIRS))
        return [SampleCase("u=1 pairs fp32 B=8", logits, one, seeds, 0),
                SampleCase("u=1 pairs bf16 B=40", logits.to(torch.bfloat16).repeat(5, 1), one.repeat(5),
                           seeds.repeat(5), 0)]
    return cached("u1", make)


def greedy_tie_case(V: int, dtype) -> SampleCase:
    """Greedy rows whose maximum sits at several indices: inside one 16-byte vector, on two
    threads of a wave, on two waves, in two chunks of the split path, first and last element.
    The answer is the lowest planted index."""
    g = _gen(V)
    plants = [(3, 4), (7, 8), (8, 8 + 64), (5, 8 * 64 + 5), (8 * 1024 - 1, 8 * 1024), (2, 8 * 1024 + 2),
              (SP_CHUNK - 1, SP_CHUNK), (SP_CHUNK + 9, 2 * SP_CHUNK + 1), (513, 2 * SP_CHUNK - 1, 2 * SP_CHUNK),
              (0, V - 1), (V - 2, V - 1), (V - 9, V - 1), (1, V // 2, V - 1)]
    plants = [tuple(sorted({i for i in p if 0 <= i < V})) for p in plants]
    plants = [p for p in plants if len(p) > 1]
    logits = torch.randn(len(plants), V, generator=g).clamp(max=3.0).to(dtype)
    for b, p in enumerate(plants):
        logits[b, list(p)] = 4.0
    B = len(plants)
    return SampleCase(f"greedy ties V={V}", logits, torch.zeros(B), torch.arange(B, dtype=torch.long), 0)


def views(t: torch.Tensor):
    """(name, view) of a [B, V] tensor with equal contents: contiguous; rows of a wider buffer with
    an odd row stride (scalar loads); rows of a wider buffer with a row stride that is a multiple
    of 8 (16-byte loads, a scalar tail when V % 8 != 0); the same stride with the base one element
    into the buffer (16-byte loads only if the pointer is checked too)."""
    B, V = t.shape
    yield "contiguous", t
    S = V + 3 if V % 2 == 0 else V + 2
    wide = torch.zeros(B, S, dtype=t.dtype, device=t.device)
    wide[:, :V] = t
    yield "odd stride", wide[:, :V]
    S8 = (V + 8 + 7) // 8 * 8
    wide8 = torch.zeros(B, S8, dtype=t.dtype, device=t.device)
    wide8[:, :V] = t
    yield "stride % 8 == 0, aligned", wide8[:, :V]
    flat = torch.zeros(B * S8 + 8, dtype=t.dtype, device=t.device)
    v = flat.as_strided((B, V), (S8, 1), 1)
    v.copy_(t)
    yield "stride % 8 == 0, base + 1", v


# ---------------------------------------------------------------------------------------------
# thresholds
# ---------------------------------------------------------------------------------------------

@dataclass
class Thresh:
    thresh: float          # smallest kept value, or -inf when every finite value is kept
    gap: float             # relative distance of mass_gt(v) from top_p * Z_k at the two values by the cut
    sep: float             # smallest distance between a cut value and its neighbours / row range
    kept: int              # number of kept elements


def _distinct(row: torch.Tensor):
    x = row.detach().cpu().double().flatten()
    fin = x[torch.isfinite(x)]
    d, cnt = torch.unique(fin, return_counts=True)
    return d.flip(0), cnt.flip(0)


def threshold64(row: torch.Tensor, T: float, k: int, p: float) -> Thresh:
    """The keep rule of ``ops.topkp_threshold`` per distinct value in float64: v is kept iff
    ``#{u > v} < k`` and ``sum_{u > v} exp((u - max) / T) <= p * Z_k``, Z_k the mass of the values
    passing the count condition.  ``p`` is taken as the fp32 number the kernel reads."""
    V = row.numel()
    p = float(torch.tensor(p, dtype=torch.float32))
    T = float(torch.tensor(T, dtype=torch.float32))
    kk = V if (k <= 0 or k > V) else k
    d, cnt = _distinct(row)
    n = d.numel()
    if T <= 1e-5 or (kk >= V and p >= 1.0) or n == 0:
        return Thresh(NEG_INF, math.inf, math.inf, V)
    cnt_gt = cnt.cumsum(0) - cnt
    e = torch.exp((d - d[0]) / T) * cnt
    mass_gt = e.cumsum(0) - e
    in_k = cnt_gt < kk
    nk = int(in_k.sum())
    pz = p * float(e[:nk].sum())
    keep = in_k & (mass_gt <= pz)
    nkeep = int(keep.sum())
    assert bool(keep[:nkeep].all())                       # the kept set is a prefix
    gap = math.inf
    if p < 1.0:
        for j in (nkeep - 1, nkeep):
            if 0 <= j < nk:
                gap = min(gap, abs(float(mass_gt[j]) - pz) / pz)
    rng = float(d[0] - d[-1])
    sep = math.inf
    for j in {nk - 1, nkeep - 1}:
        for a, b in ((j - 1, j), (j, j + 1)):
            if 0 <= a and b < n and rng > 0:
                sep = min(sep, float(d[a] - d[b]) / rng)
    if nkeep == n:
        return Thresh(NEG_INF, gap, sep, V)
    return Thresh(float(d[nkeep - 1]), gap, sep, int(cnt[:nkeep].sum()))


def mid_p(row: torch.Tensor, T: float, k: int, j: int) -> float:
    """``top_p`` (an fp32 number) that keeps the ``j + 1`` largest distinct values of the top-k set
    (fewer if the last of them weighs under 4e-3 of the kept mass) and sits half-way between the
    cumulative masses on either side of that cut; 1.0 if the top-k set has fewer than two distinct
    values."""
    V = row.numel()
    kk = V if (k <= 0 or k > V) else k
    d, cnt = _distinct(row)
    cnt_gt = cnt.cumsum(0) - cnt
    nk = int((cnt_gt < kk).sum())
    if nk < 2:
        return 1.0
    e = torch.exp((d - d[0]) / float(torch.tensor(T, dtype=torch.float32))) * cnt
    mass_gt = e.cumsum(0) - e
    for j in range(max(0, min(j, nk - 2)), -1, -1):     # a cut further up if the value below it weighs too little
        pz = 0.5 * float(mass_gt[j] + mass_gt[j + 1])
        if 0.5 * float(e[j]) / pz >= 2 * MIN_GAP:
            break
    return float(torch.tensor(pz / float(e[:nk].sum()), dtype=torch.float32))


@dataclass
class ThreshCase:
    name: str
    logits: torch.Tensor
    temps: torch.Tensor
    top_k: torch.Tensor
    top_p: torch.Tensor
    rows: list                 # what each row is there for
    ref: list                  # Thresh per row


THRESH_V = [8, 100, 1000, 4099, 32768]


def _zipf_row(V, dtype, g, a=1.1):
    """log of probabilities ~ 1 / rank^a in random order, shifted so that no value is near 0."""
    lp = -a * torch.log(torch.arange(1, V + 1, dtype=torch.float64)) + 4.25
    return lp[torch.randperm(V, generator=g)].to(dtype)


def thresh_case(V: int, dtype) -> ThreshCase:
    def make():
        g = _gen(V + (1 if dtype == torch.float32 else 0))
        rows, logits, temps, ks, ps = [], [], [], [], []

        def add(name, row, T, k, p):
            rows.append(name)
            logits.append(row)
            temps.append(T)
            ks.append(k)
            ps.append(p)

        def srt(row):
            return row.double().sort(descending=True, stable=True)

        # top-k only; the k-th value also sits at ranks k + 1 and k + 2: all three are kept
        k = max(2, min(5, V // 2))
        r = _zipf_row(V, dtype, g)
        _, order = srt(r)
        r[order[k:k + 2]] = float(r[order[k - 1]])
        add("top-k only, ties straddle the cut", r, 1.0, k, 1.0)
        add("k = 1", _zipf_row(V, dtype, g), 0.7, 1, 1.0)
        r = _zipf_row(V, dtype, g)
        r[srt(r)[1][-1]] = r.double().min() - 1.0               # one strictly smallest element
        add("k = V - 1", r, 1.3, V - 1, 1.0)
        r = _zipf_row(V, dtype, g)
        add("k > V, top-p", r, 1.0, V + 5, mid_p(r, 1.0, V + 5, 3))
        r = _zipf_row(V, dtype, g)
        add("k = V, top-p", r, 0.7, V, mid_p(r, 0.7, V, 1))
        r = _zipf_row(V, dtype, g)
        add("top-p keeps the maximum only", r, 1.0, 0, mid_p(r, 1.0, 0, 0))
        add("p = 1 with top-k", _zipf_row(V, dtype, g), 1.3, min(10, V - 1), 1.0)
        r = _zipf_row(V, dtype, g)
        r[V - V // 3:] = NEG_INF
        add("-inf tail, top-k then top-p", r, 1.0, 4, mid_p(r, 1.0, 4, 2))
        r = _zipf_row(V, dtype, g)
        r[V - V // 3:] = NEG_INF
        add("-inf tail, k above the finite count", r, 0.7, V - 1, mid_p(r, 0.7, V - 1, 2))
        add("constant row", torch.full((V,), 1.5, dtype=dtype), 1.0, 3, 0.5)
        add("greedy row", _zipf_row(V, dtype, g), 0.0, 3, 0.5)
        r = _zipf_row(V, dtype, g)
        kk = min(20, V - 1)
        add("top-p cut inside the top-k set", r, 1.3, kk, mid_p(r, 1.3, kk, 4))
        add("no filter", _zipf_row(V, dtype, g), 1.0, 0, 1.0)
        r = _zipf_row(V, dtype, g)
        add("top-p only, 12 values", r, 0.7, 0, mid_p(r, 0.7, 0, 11))
        add("greedy row, filter off", _zipf_row(V, dtype, g), 0.0, 0, 1.0)
        c = ThreshCase(f"V={V} {'bf16' if dtype == torch.bfloat16 else 'fp32'}", torch.stack(logits),
                       torch.tensor(temps, dtype=torch.float32), torch.tensor(ks, dtype=torch.long),
                       torch.tensor(ps, dtype=torch.float32), rows, [])
        c.ref = [threshold64(c.logits[b], float(c.temps[b]), int(c.top_k[b]), float(c.top_p[b]))
                 for b in range(len(rows))]
        for name, t in zip(rows, c.ref):
            assert t.gap >= MIN_GAP, (c.name, name, t.gap)
            assert t.sep > 4 * SEARCH_WIDTH, (c.name, name, t.sep)
        return c
    return cached(("thresh", V, dtype), make)


def superset_case():
    """fp32 values closer than range / 16^6 at the cut (the documented exception): four
    consecutive floats around 1.0 in a row of range 20, top_k cutting through them.  Returns
    (logits [1, V], temps, top_k, top_p, reference threshold, range)."""
    V = 1000
    g = _gen(77)
    row = (torch.rand(V, generator=g) * 9.0 - 10.0).float()          # background in [-10, -1)
    row[0], row[1] = 10.0, -10.0                                      # range exactly 20
    top = torch.tensor([9.0, 8.0, 7.0]).float()
    row[10:13] = top
    v = torch.tensor(1.0)
    cluster = [float(v)]
    for _ in range(3):
        v = torch.nextafter(v, torch.tensor(2.0))
        cluster.append(float(v))
    row[[500, 20, 731, 64]] = torch.tensor(cluster)
    k = 6                                                             # 10, 9, 8, 7 and the two largest of the cluster
    ref = threshold64(row, 1.0, k, 1.0)
    assert ref.thresh == cluster[2] and (cluster[3] - cluster[0]) < 20.0 * SEARCH_WIDTH
    return (row[None], torch.ones(1), torch.tensor([k]), torch.ones(1), ref.thresh, 20.0)


# ---------------------------------------------------------------------------------------------
# top-k and top-k log-probs
# ---------------------------------------------------------------------------------------------

def topk_ref(values: torch.Tensor, k: int):
    """The first k of a stable sort by (-value, index), in float64."""
    v, i = values.detach().cpu().double().sort(dim=-1, descending=True, stable=True)
    return v[:, :k], i[:, :k]


def logprobs64(logits: torch.Tensor) -> torch.Tensor:
    return torch.log_softmax(logits.detach().cpu().double(), dim=-1)


TOPK_K = [1, 2, 8, 16]
TOPK_V = [16, 17, 255, 2055, 32000]
TKL_K = [1, 2, 3, 4, 5, 8]
TKL_V = [8, 2047, 2048, 2049, 4103, 32768]


def topk_rows(V: int, dtype, chunk_ties=()) -> tuple:
    """([B, V] logits, row names): random rows (bf16 ties are frequent), a constant row, a -inf
    tail that leaves 3 finite values, planted ties, rows of magnitude 3e4 and one of magnitude 1e-6."""
    def make():
        g = _gen(31 * V + (1 if dtype == torch.float32 else 0))
        names, rows = [], []
        for s in (1.0, 3.0):
            names.append(f"N(0, {s})")
            rows.append(torch.randn(V, generator=g) * s)
        names.append("constant")
        rows.append(torch.full((V,), -2.5))
        r = torch.randn(V, generator=g)
        r[3:] = NEG_INF
        names.append("-inf tail after 3 values")
        rows.append(r)
        r = torch.randn(V, generator=g)
        r[V - V // 4:] = NEG_INF
        names.append("-inf tail, last quarter")
        rows.append(r)
        r = torch.randn(V, generator=g).clamp(max=2.0)
        idx = sorted({0, 1, V // 2, V - 1, V - 2, 7 % V, 8 % V, *[i for i in chunk_ties if i < V]})
        r[idx] = 5.0
        names.append("maximum planted at " + ",".join(map(str, idx)))
        rows.append(r)
        names.append("ascending to 3e4")                              # every element raises the running maximum
        rows.append(torch.linspace(-3e4, 3e4, V) if V > 1 else torch.tensor([3e4]))
        names.append("descending from 3e4")
        rows.append(torch.linspace(3e4, -3e4, V) if V > 1 else torch.tensor([3e4]))
        r = torch.randn(V, generator=g) * 3
        names.append("ascending N(0, 3)")
        rows.append(r.sort().values)
        r = torch.where(torch.rand(V, generator=g) < 0.5, torch.tensor(-3e4), torch.tensor(3e4))
        names.append("+-3e4 at random")
        rows.append(r + torch.randn(V, generator=g) * 200)
        # distinct bf16 values whose log-probs (about -log V) coincide in fp32: the order is the logits'
        names.append("near-zero logits")
        rows.append(torch.randn(V, generator=g) * 1e-6)
        return torch.stack(rows).to(dtype), names
    return cached(("topk", V, dtype, tuple(chunk_ties)), make)


# ---------------------------------------------------------------------------------------------
# draft trees
# ---------------------------------------------------------------------------------------------

@dataclass
class TreeCase:
    name: str
    parent: torch.Tensor       # int32 [B, N]
    draft: torch.Tensor        # int64 [B, N]
    target: torch.Tensor       # int64 [B, N]
    max_path: int
    expect_accept: Optional[list] = None      # hand-made trees: the accept length known by construction
    expect_best: Optional[list] = None        # ... and the last node of the path


def _depths(par):
    d = [0] * len(par)
    for n in range(1, len(par)):
        d[n] = d[par[n]] + 1
    return d


def brute_tree(c: TreeCase, parent_only: bool = False, tie_high: bool = False):
    """(anc [B, 64], depth [B, N], accept_len [B], path [B, max_path], tokens [B, max_path + 1]) by
    walking every root-to-leaf path downwards.  ``parent_only`` / ``tie_high``: the slips "a
    node is accepted when it matches its parent's target" and "the highest index wins a tie"."""
    par_all, dr_all, tg_all = c.parent.tolist(), c.draft.tolist(), c.target.tolist()
    B, N = c.parent.shape
    anc = torch.zeros(B, 64, dtype=torch.long)
    depth = torch.zeros(B, N, dtype=torch.int32)
    acc = torch.zeros(B, dtype=torch.int32)
    path = torch.zeros(B, c.max_path, dtype=torch.int32)
    toks = torch.zeros(B, c.max_path + 1, dtype=torch.long)
    for b in range(B):
        par, dr, tg = par_all[b], dr_all[b], tg_all[b]
        kids = [[] for _ in range(N)]
        for n in range(1, N):
            kids[par[n]].append(n)
        accepted = []                       # (depth, node, path to node)
        stack = [(0, [0], True)]
        while stack:
            n, pth, ok = stack.pop()
            bits = sum(1 << i for i in pth)
            anc[b, n] = bits - (1 << 64) if bits >= 1 << 63 else bits
            depth[b, n] = len(pth) - 1
            if ok:
                accepted.append((len(pth) - 1, n, pth))
            for ch in kids[n]:
                m = dr[ch] == tg[n]
                stack.append((ch, pth + [ch], m if parent_only else (ok and m)))
        dmax = max(d for d, _, _ in accepted)
        ends = [(n, p) for d, n, p in accepted if d == dmax]
        best, pth = max(ends) if tie_high else min(ends)
        acc[b] = dmax
        for k_, node in enumerate(pth):
            if k_ < c.max_path:
                path[b, k_] = node
                if k_ > 0:
                    toks[b, k_ - 1] = dr[node]
        if dmax < c.max_path + 1:
            toks[b, dmax] = tg[best]
    return anc, depth, acc, path, toks


def _random_tree_case(N: int, B: int = 5) -> TreeCase:
    rng = random.Random(100 + N)
    par = [[-1] + [rng.randrange(0, n) for n in range(1, N)] for _ in range(B)]
    target = [[rng.randrange(0, 5) for _ in range(N)] for _ in range(B)]
    draft = [[7] + [target[b][par[b][n]] if rng.random() < 0.7 else 5 + rng.randrange(0, 3) for n in range(1, N)]
             for b in range(B)]
    mp = max(max(_depths(p)) for p in par) + 1
    return TreeCase(f"random B={B} N={N}", torch.tensor(par, dtype=torch.int32), torch.tensor(draft),
                    torch.tensor(target), mp)


def _hand(name, par, draft, target, accept, best, max_path=None):
    mp = max(_depths(par)) + 1 if max_path is None else max_path
    return TreeCase(name, torch.tensor([par], dtype=torch.int32), torch.tensor([draft]), torch.tensor([target]), mp,
                    [accept], [best])


def tree_cases() -> list:
    def make():
        cs = [_random_tree_case(N) for N in (1, 2, 7, 33, 64)]
        # a chain of 64 nodes, all accepted: depth 63 = max_path - 1, and anc[63] has bit 63 next to every low bit
        chain = [-1] + list(range(63))
        tgt = [100 + n for n in range(64)]
        cs.append(_hand("chain of 64, all accepted", chain, [9] + tgt[:63], tgt, 63, 63))
        # the same chain broken at node 40; node 41.. still match their parents
        d = [9] + tgt[:63]
        d[40] = 5
        cs.append(_hand("chain of 64, node 40 fails, its descendants match their parents", chain, d, tgt, 39, 39))
        # node 63 hangs off the root next to a chain 0-1-..-62 that fails at once: bit 63 with bit 0 only
        par = [-1] + list(range(62)) + [0]
        d = [9, 5] + tgt[1:62] + [tgt[0]]
        cs.append(_hand("bit 63 accepted next to a failed chain", par, d, tgt, 1, 63))
        # a star: the root and 63 leaves; leaves 17 and 40 match, the lowest index wins
        par = [-1] + [0] * 63
        d = [9] + [5] * 63
        d[17] = d[40] = tgt[0]
        cs.append(_hand("star, two matching leaves", par, d, tgt, 1, 17))
        # two accepted leaves of equal depth 2 in different branches: 0-2-5 and 0-1-4 (and 0-1-3 failing)
        par = [-1, 0, 0, 1, 1, 2]
        tg = [10, 11, 12, 13, 14, 15]
        cs.append(_hand("two accepted leaves of equal depth", par, [9, 10, 10, 5, 11, 12], tg, 2, 4))
        # 0-1-2-3: node 1 fails, nodes 2 and 3 match their parents' targets; 0-4 is the accepted branch
        par = [-1, 0, 1, 2, 0]
        cs.append(_hand("matches under a failed ancestor are rejected", par, [9, 5, 11, 12, 10], tg[:5], 1, 4))
        # nothing matches: the root alone, the bonus token is the root's target
        cs.append(_hand("root only", [-1, 0, 0, 1], [9, 5, 5, 5], tg[:4], 0, 0))
        # accept depth = max_path - 1 on the deepest branch of a bushy tree
        par = [-1, 0, 0, 1, 1, 3, 5, 2]
        cs.append(_hand("accept depth = max_path - 1", par, [9, 10, 10, 11, 11, 13, 15, 5], [10, 11, 12, 13, 14, 15, 16, 17],
                        4, 6))
        return cs
    return cached("tree", make)


# ---------------------------------------------------------------------------------------------
# an fp32 model of the sampling kernels with switchable slips
# ---------------------------------------------------------------------------------------------

MUTANTS = ["hash of i + 1", "last V % 8 elements dropped", "chunk offset not added", "ties to the higher index",
           "v <= thresh skipped", "temperature not applied"]


def _argbest(score: torch.Tensor, high: bool) -> int:
    m = (score == score.max()).nonzero().flatten()
    return int(m[-1] if high else m[0])


def kernel_model(c: SampleCase, mutate: Optional[str] = None) -> torch.Tensor:
    """Picks of an fp32 sampler for ``c`` (thresholds from the float64 reference), correct with
    ``mutate=None`` and otherwise with that one slip."""
    assert mutate is None or mutate in MUTANTS
    B, V = c.logits.shape
    lf = c.logits.float()
    h = hash_bits(c.seeds, c.step, V, id_shift=1 if mutate == "hash of i + 1" else 0)
    u = ops._uniform_from_hash(h)
    th = c.thresholds()
    out = []
    for b in range(B):
        T = float(c.temps[b])
        row = lf[b]
        if T <= 1e-5:
            score = row.clone()
        else:
            t = torch.tensor(1.0 if mutate == "temperature not applied" else T)
            score = row / t - torch.log(-torch.log(u[b]))
            drop = row <= th[b] if mutate == "v <= thresh skipped" else row < th[b]
            score[drop] = NEG_INF
        if mutate == "last V % 8 elements dropped" and V >= 8:
            score = score[: V - V % 8]
        if bool(torch.isinf(score).all()):
            out.append(0)
            continue
        i = _argbest(score, mutate == "ties to the higher index")
        if mutate == "chunk offset not added" and V >= 2 * SP_CHUNK:
            i %= SP_CHUNK
        out.append(i)
    return torch.tensor(out, dtype=torch.long)


def topk_model(values: torch.Tensor, k: int, mutate: Optional[str] = None, chunk: int = 0):
    """Top-k of an fp32 kernel model: correct, or with one of the slips that apply to a top-k."""
    v = values.detach().cpu().float()
    B, V = v.shape
    if mutate == "last V % 8 elements dropped" and V - V % 8 >= k:
        v = v[:, : V - V % 8]
    if mutate == "ties to the higher index":
        s, i = v.flip(-1).sort(dim=-1, descending=True, stable=True)
        i = v.shape[1] - 1 - i
    else:
        s, i = v.sort(dim=-1, descending=True, stable=True)
    s, i = s[:, :k], i[:, :k]
    if mutate == "chunk offset not added" and chunk:
        i = i % chunk
    return s, i
