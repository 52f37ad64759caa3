"""Row padding for the MLP GEMMs from a table measured on this GPU at start-up.

hipBLASLt picks its kernel from (M, N, K), and on MI355X the choice has
cliffs: for the Llama-3-70B down-projection (N 8192, K 28672) M = 1792 runs
in 755 us while M = 1800 runs in 621 us; the QKV GEMM takes 301 us at
M = 1700 and 243 us at M = 1800 (profiles/r1_gemm_m_sweep_70b.md).  A serving
step's row count is whatever the scheduler packed, so it lands on both sides
of those cliffs.

The MLP is row-independent, so its rows can be padded for free as far as
correctness goes: ``MlpPadTable.measure`` times gate_up + SiLU·mul + down for
every multiple of ``step`` rows up to the token budget, and ``pad(T)`` returns
the row count (a multiple of ``step``, at most ``max_grow`` larger than T)
with the lowest measured time.  ``LlamaModel.forward_layers`` then lets the
o-projection write into a padded buffer and runs the MLP on the padded rows.

Each half of the MLP is measured with both GEMM implementations — hipBLASLt
(+ the separate silu_mul pass) and the hand-written LDS-tiled MFMA kernel
(``ops.mfma_gemm``: gate_up with the SwiGLU epilogue fused, down as a plain
GEMM) — and ``impl(rows)`` tells the model which one is faster at that row
count on this GPU (``DGI_MFMA_GEMM=0`` keeps hipBLASLt everywhere, ``=force``
the MFMA kernel wherever it applies).  The QKV and o projections get the same
per-row-count choice (``proj_impl(rows)``, at the first grid point >= rows): with
the ping-pong kernel and its split-K remainder (``ops.mfma_gemm``) the
hand-written kernel beats hipBLASLt on several of their row counts.
"""
from __future__ import annotations

import bisect
import os
from typing import Optional

import torch


MFMA_GEMM = os.environ.get("DGI_MFMA_GEMM", "1")
# the MFMA kernel must beat hipBLASLt by 3 % to be chosen: near-ties would otherwise flip
# between runs on timing noise (same speed either way, less reproducible: VERDICT r4 weak #1)
MFMA_MARGIN = 0.97
# The table ships with the package (dgi/tuned/, measured on MI355X: median of several passes)
# so a fresh box routes every row count the same way as the box that measured it, and skips
# the start-up measurement.  DGI_GEMM_TABLE=measure re-measures; DGI_GEMM_TABLE_SAVE=<path>
# writes the measured table (scripts/gemm_table_build.py combines passes into the shipped one).
TABLE_MODE = os.environ.get("DGI_GEMM_TABLE", "auto")
TUNED_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tuned")
# "q" / "o": entries of tables saved while the qkv / o-proj could join the padded rows; never
# measured now (null in the shipped table), still read
RAW_KEYS = ("front", "front_mfma", "back", "back_mfma", "q", "o", "pq_blas", "pq_mfma", "po_blas", "po_mfma")


class MlpPadTable:
    def __init__(self, grid: list, times: list, step: int, max_grow: float = 0.15, impls: Optional[list] = None,
                 proj_impls: Optional[list] = None, raw: Optional[list] = None):
        self.grid = list(grid)
        self.times = list(times)
        self.step = step
        self.max_grow = max_grow
        # per grid point: (gate_up via MFMA+SwiGLU?, down via MFMA?)
        self.impls = list(impls) if impls is not None else [(False, False)] * len(self.grid)
        # per grid point: (QKV via MFMA?, o-proj via MFMA?)
        self.proj_impls = list(proj_impls) if proj_impls is not None else [(False, False)] * len(self.grid)
        # per grid point: the measured times (RAW_KEYS, ms; None = not measured) behind the choices
        self.raw = list(raw) if raw is not None else None
        self.source = "measured"
        self._cache: dict = {}

    @classmethod
    def decide(cls, grid: list, raw: list, step: int, margin: float = None, force: bool = False) -> "MlpPadTable":
        """Implementation choices and padding objective from raw per-implementation times: the
        MFMA kernel where it beats hipBLASLt by ``1 - margin`` (or everywhere with ``force``)."""
        margin = MFMA_MARGIN if margin is None else margin
        times, impls, proj = [], [], []

        def pick(blas, mfma):
            if mfma is None:
                return blas, False
            if force or mfma < blas * margin:
                return mfma, True
            return blas, False

        for r in raw:
            f, fm = pick(r["front"], r.get("front_mfma"))
            b, bm = pick(r["back"], r.get("back_mfma"))
            times.append(f + b + (r.get("q") or 0.0) + (r.get("o") or 0.0))
            impls.append((fm, bm))
            pq = r.get("pq_mfma") is not None and pick(r["pq_blas"], r["pq_mfma"])[1]
            po = r.get("po_mfma") is not None and pick(r["po_blas"], r["po_mfma"])[1]
            proj.append((pq, po))
        return cls(grid, times, step, impls=impls, proj_impls=proj, raw=raw)

    @staticmethod
    def median_raw(runs: list) -> list:
        """Element-wise median of several passes' raw times (same grid)."""
        import statistics
        out = []
        for pts in zip(*runs):
            d = {}
            for k in RAW_KEYS:
                v = [p[k] for p in pts if p.get(k) is not None]
                d[k] = statistics.median(v) if v else None
            out.append(d)
        return out

    def to_json(self, key: dict) -> dict:
        return {"key": key, "grid": self.grid, "step": self.step, "raw": self.raw, "margin": MFMA_MARGIN}

    @classmethod
    def from_json(cls, d: dict) -> "MlpPadTable":
        t = cls.decide(d["grid"], d["raw"], d["step"], margin=d.get("margin"))
        t.source = "shipped"
        return t

    @classmethod
    def measure(cls, gate_up: torch.Tensor, down: torch.Tensor, m_min: int = 512, m_max: int = 4096,
                step: int = 32, reps: int = 3, proj_qkv: Optional[torch.Tensor] = None,
                proj_o: Optional[torch.Tensor] = None) -> "MlpPadTable":
        """``proj_qkv`` / ``proj_o``: the (bias-free) QKV and o-proj weights whose
        implementation is chosen per row count (``proj_impl``)."""
        from dgi import ops
        H = gate_up.shape[1]
        x = torch.randn(m_max, H, device=gate_up.device, dtype=gate_up.dtype) * 0.1
        a = torch.randn(m_max, gate_up.shape[0] // 2, device=gate_up.device, dtype=gate_up.dtype) * 0.1
        pa = torch.randn(m_max, proj_o.shape[1], device=gate_up.device, dtype=gate_up.dtype) * 0.1 \
            if proj_o is not None else None
        grid = list(range(m_min, m_max + 1, step))
        raw = []
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        use_mfma = MFMA_GEMM != "0" and ops.mfma_gemm_ok(x, gate_up)
        mfma_down = use_mfma and ops.mfma_gemm_ok(a, down)
        force = MFMA_GEMM == "force"

        def timed(fn):
            fn()
            best = float("inf")
            for _ in range(reps):
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                best = min(best, e0.elapsed_time(e1))
            return best

        for m in grid:
            r = dict.fromkeys(RAW_KEYS)
            r["front"] = timed(lambda: ops.silu_mul(ops.linear(x[:m], gate_up)))
            r["back"] = timed(lambda: ops.linear(a[:m], down))
            if use_mfma:
                r["front_mfma"] = timed(lambda: ops.mfma_gemm(x[:m], gate_up, 1))
            if mfma_down:
                r["back_mfma"] = timed(lambda: ops.mfma_gemm(a[:m], down, 0))
            if use_mfma and proj_qkv is not None and ops.mfma_gemm_ok(x, proj_qkv):
                r["pq_mfma"] = timed(lambda: ops.mfma_gemm(x[:m], proj_qkv, 0))
                r["pq_blas"] = timed(lambda: ops.linear(x[:m], proj_qkv))
            if use_mfma and proj_o is not None and ops.mfma_gemm_ok(pa, proj_o):
                r["po_mfma"] = timed(lambda: ops.mfma_gemm(pa[:m], proj_o, 0))
                r["po_blas"] = timed(lambda: ops.linear(pa[:m], proj_o))
            raw.append(r)
        return cls.decide(grid, raw, step, force=force)

    def impl(self, rows: int) -> tuple:
        """(gate_up via the fused MFMA SwiGLU kernel, down via the MFMA kernel) at ``rows``."""
        if not self.grid or not (self.grid[0] <= rows <= self.grid[-1]):
            return False, False
        i = bisect.bisect_left(self.grid, rows)
        return self.impls[i] if self.grid[i] == rows else (False, False)

    def proj_impl(self, rows: int) -> tuple:
        """(QKV via the MFMA kernel, o-proj via the MFMA kernel) at ``rows`` (first grid point >= rows)."""
        if not self.grid or not (self.grid[0] <= rows <= self.grid[-1]):
            return False, False
        return self.proj_impls[bisect.bisect_left(self.grid, rows)]

    # the two RMSNorm kernels a fused-norm layer removes, priced from their HBM traffic (read x and
    # the residual, write both: 8 bytes per element each) plus a launch ramp; the round-2 profile
    # measured 30.7 us per call at ~1,900 rows of the 70B stream (profiles/r2_70b_1gpu_kernel_stats.md)
    NORM_HBM_TBS = 5.0
    NORM_RAMP_MS = 0.004

    def fold(self, rows: int, hidden: int = 8192) -> bool:
        """Run the fused-norm layers at ``rows``?  Yes when the all-MFMA layer (qkv, o, gate_up,
        down on the ping-pong kernel) costs no more than the best per-projection mix plus the
        two norm kernels the fusion removes (first grid point >= rows)."""
        if not self.raw or not self.grid or not (self.grid[0] <= rows <= self.grid[-1]):
            return False
        r = self.raw[bisect.bisect_left(self.grid, rows)]
        keys = ("front", "front_mfma", "back", "back_mfma", "pq_blas", "pq_mfma", "po_blas", "po_mfma")
        if any(r.get(k) is None for k in keys):
            return False
        mfma = r["front_mfma"] + r["back_mfma"] + r["pq_mfma"] + r["po_mfma"]
        best = (min(r["front"], r["front_mfma"]) + min(r["back"], r["back_mfma"]) + min(r["pq_blas"], r["pq_mfma"])
                + min(r["po_blas"], r["po_mfma"]))
        norms = 2 * (self.NORM_RAMP_MS + rows * hidden * 8 / (self.NORM_HBM_TBS * 1e9))
        return mfma <= best + norms

    def pad(self, T: int) -> int:
        """Rows to run the MLP on for a step of ``T`` rows (``T`` when the table has no say)."""
        r = self._cache.get(T)
        if r is not None:
            return r
        r = T
        if self.grid and self.grid[0] <= T <= self.grid[-1]:
            i = bisect.bisect_left(self.grid, T)            # first grid row count >= T
            j = i
            best = i
            while j < len(self.grid) and self.grid[j] <= T * (1 + self.max_grow):
                if self.times[j] < self.times[best]:
                    best = j
                j += 1
            r = self.grid[best]
        self._cache[T] = r
        return r


_TABLES: dict = {}      # (shapes, device, step) -> (m_max, table): one measurement per process


def table_key(model, step: int, m_min: int) -> dict:
    L = model.layers[0]
    # "qkv_pad" / "oproj_pad": switches that are gone; the literals keep the shipped table's key and name
    return {"gate_up": list(L.gate_up.shape), "down": list(L.down.shape), "qkv": list(L.qkv.shape),
            "o": list(L.o.shape), "qkv_bias": L.qkv_bias is not None, "step": step, "m_min": m_min,
            "qkv_pad": False, "oproj_pad": False, "mfma": MFMA_GEMM}


def tuned_path(key: dict) -> str:
    import hashlib
    import json
    h = hashlib.sha1(json.dumps(key, sort_keys=True).encode()).hexdigest()[:12]
    return os.path.join(TUNED_DIR, f"gemm_table_{key['gate_up'][1]}x{key['down'][1]}_{h}.json")


def device_tag(device=None) -> dict:
    """What a measured routing table is only valid on: the GPU architecture (``gfx950``,
    without feature suffixes) and the HIP major.minor of the torch build (hipBLASLt's
    kernels change between releases).  Stored next to the key in every saved table and
    compared on load (the key alone let any device reuse the MI355X choices)."""
    arch, hip = None, None
    if torch.cuda.is_available():
        props = torch.cuda.get_device_properties(device if device is not None else torch.cuda.current_device())
        arch = str(getattr(props, "gcnArchName", "")).split(":")[0] or None
    if torch.version.hip:
        hip = ".".join(torch.version.hip.split(".")[:2])
    return {"arch": arch, "hip": hip}


def load_tuned(key: dict, m_max: int, device=None) -> Optional[MlpPadTable]:
    import json
    p = tuned_path(key)
    if not os.path.exists(p):
        return None
    with open(p) as f:
        d = json.load(f)
    if d.get("key") != key or not d["grid"] or d["grid"][-1] < m_max:
        return None
    if d.get("device") != device_tag(device):      # another GPU / ROCm: measure its own table
        return None
    return MlpPadTable.from_json(d)


M_MIN = 256        # first row count of the table (part of the shipped table's key)


def build_for_model(model, m_max: int, step: int = 32) -> Optional[MlpPadTable]:
    """The routing / padding table for ``model``'s projection shapes on its device (None when
    off / not applicable): the shipped table (dgi/tuned/) when one covers ``m_max`` rows,
    else measured here.  A table already built in this process for the same weight shapes
    on the same device up to at least ``m_max`` rows is reused (the start-up capacity
    probe and the serving engine share one measurement)."""
    if os.environ.get("DGI_MLP_PAD", "1") == "0":
        return None
    layers = getattr(model, "layers", None)
    if not layers or not torch.cuda.is_available():
        return None
    L = layers[0]
    if L.gate_up.device.type != "cuda" or m_max < 1024:
        return None
    key = (tuple(L.gate_up.shape), tuple(L.down.shape), tuple(L.qkv.shape), tuple(L.o.shape), L.qkv_bias is None,
           str(L.gate_up.device), L.gate_up.dtype, step)
    hit = _TABLES.get(key)
    if hit is not None and hit[0] >= m_max:
        return hit[1]
    tk = table_key(model, step, M_MIN)
    t = load_tuned(tk, m_max, L.gate_up.device) if TABLE_MODE == "auto" else None
    if t is None:
        t = MlpPadTable.measure(L.gate_up, L.down, m_min=M_MIN, m_max=m_max, step=step,
                                proj_qkv=L.qkv if L.qkv_bias is None else None, proj_o=L.o)
        save = os.environ.get("DGI_GEMM_TABLE_SAVE")
        if save:
            import json
            with open(save, "w") as f:
                json.dump({**t.to_json(tk), "device": device_tag(L.gate_up.device)}, f)
    _TABLES[key] = (m_max, t)
    return t
