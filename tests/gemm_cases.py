"""Inputs with exactly known answers for the MFMA GEMMs (dgi/csrc/mfma_gemm.hip) and the fused
decode GEMMs (dgi/csrc/fused_decode.hip), the comparators that judge a kernel's output, a model of
the launch plan and a CPU model of the kernels with switchable slips.  No GPU needed to import.

**Exact operands.**  X is ±1 and W is ±1, ±2 (±1 above K = 512), possibly times a power of two:
every product and every partial sum is an integer multiple of one power of two below 2^24 of it, so
fp32 holds each exactly in ANY summation order, K split and fold order, and every final value is
chosen to be exactly representable in bf16 (an integer of at most 256, times that power of two).
The float64 answer must then be met bit for bit.  No entry is zero: a dropped, duplicated or
mispaired product always moves the sum.  Each case checks these conditions on its own reference
(``check``).

**Address probes** (``probe``): one-hot X rows against a W whose entries name their (n, k).

**Neighbour rule** (SwiGLU epilogues).  Gate and up are exact dyadics with |gate| <= 16; the
reference is silu(g) * u in float64 and a bf16 value b passes iff
|b - r64| <= half a bf16 ulp of r64 + DELTA * |r64|.  DELTA is taken from no kernel: it is 16 x
``FP32_GAP``, the largest relative distance between the fp32 CPU evaluation (``ops.silu_mul_ref``
on the exact g, u) and float64 over the committed cases.  The factor covers the kernels' ``__expf``
(hardware exp2 of a rounded product, whose error grows with |g|) and their division.  An element is
*decisive* when exactly one bf16 value passes; at most 1 % of a case's elements may be non-decisive.

**Normalised epilogues.**  eps = 0 and the partial sums of squares of row m add up to K * 4^-j,
j = m % 3 (every other column holds a 32nd of it plus a small distinct value, column 0 the rest), so that
rstd = 2^j if the hardware rsqrt is exact at powers of four, and everything downstream is exact.

**RoPE.**  ``quarter_table`` holds quarter-turn rotations only ((cos, sin) one of (1, 0), (0, 1),
(-1, 0), (0, -1), varying with the position and the frequency index), so q, k and the paged caches
are exact and the pair (d, d + 64), the sign, the position lookup, the head offset, the slot and
the rows with slot -1 are all pinned.

**Residual epilogue.**  Y is integers, a quarter of them plus one half: where |Y + acc| >= 128 such a
value is a tie between two bf16 neighbours, so round-to-nearest-even is pinned against truncation and
the row statistics of the STORED values differ from those of the fp32 sums.  Four times every partial
sum of squares is an integer below 2^24: ``ss`` must be bit-equal too.
"""
import types

import torch

BF = torch.bfloat16
SENT = -77.0                 # fill of every output buffer; PAD columns / rows around the written window
PAD = 8
TAIL = 2                     # sentinel rows below row M - 1

# max |silu_mul_ref_fp32 - r64| / |r64| over swiglu_cpu_cases(): 1.695e-7 as measured by
# test_gemm_exact_cpu.py::test_fp32_gap_is_the_recorded_one, which fails if the measurement leaves
# [0.95, 1] x this figure
FP32_GAP = 1.70e-7
DELTA = 16 * FP32_GAP
MAX_NON_DECISIVE = 0.01

MUTATIONS = ("drop_k", "swap_chunks", "truncate", "round_piece", "skip_piece", "row_past_m", "ss_fp32", "short_ss",
             "partner32", "sin_sign", "swap_gate_up")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _pick(vals, shape, g):
    return torch.tensor(vals, dtype=torch.float64)[torch.randint(0, len(vals), shape, generator=g)]


def is_bf16(t64: torch.Tensor) -> bool:
    return bool(torch.equal(t64.to(BF).double(), t64))


def to_bf16(t64: torch.Tensor) -> torch.Tensor:
    """fp64 -> fp32 (exact for every case here, asserted by ``check``) -> bf16, nearest-even."""
    return t64.float().to(BF)


def w_values(K: int):
    return (1.0, -1.0, 2.0, -2.0) if K <= 512 else (1.0, -1.0)


# ---------------------------------------------------------------------------------------------
# comparators
# ---------------------------------------------------------------------------------------------

def half_ulp(r64: torch.Tensor) -> torch.Tensor:
    """Half a bf16 ulp (8 significant bits) at r64."""
    _, e = torch.frexp(r64.abs())                    # |r| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(r64), (e - 9).clamp(min=-126 - 8))


def allowance(r64: torch.Tensor, delta: float = DELTA) -> torch.Tensor:
    return torch.where(r64 == 0, torch.zeros_like(r64), half_ulp(r64) + delta * r64.abs())


def judge(b: torch.Tensor, r64: torch.Tensor, delta: float = DELTA):
    """(elements outside the allowance, worst |b - r64| / allowance over those with one)."""
    err = (b.double() - r64).abs()
    al = allowance(r64, delta)
    bad = err > al
    pos = al > 0
    worst = float((err[pos] / al[pos]).max()) if bool(pos.any()) else 0.0
    return bad, worst


def non_decisive(r64: torch.Tensor, delta: float = DELTA) -> int:
    """Elements for which more than one bf16 value passes ``judge``."""
    b0 = to_bf16(r64)
    mag = b0.abs().view(torch.int16).to(torch.int32)
    sign = torch.where(r64 < 0, -1.0, 1.0).double()
    al = allowance(r64, delta)
    n = torch.zeros(r64.shape, dtype=torch.int32, device=r64.device)
    for step in (-1, 0, 1):
        cand = (mag + step).clamp(min=0).to(torch.int16).view(BF).double() * sign
        n += (((cand - r64).abs() <= al) & (mag + step >= 0)).int()
    return int((n > 1).sum())


def verdict(c, y, ss=None, kc=None, vc=None, res_out=None, delta: float = DELTA):
    """Judge a kernel's outputs for case c: (failures, worst neighbour-rule ratio).  y is the whole
    sentinel buffer [M + TAIL, PAD + cols + PAD]; the kernel was given y[:M, PAD:PAD + cols]."""
    fails, worst = [], 0.0
    M, wc = c.M, c.wcols
    outside = torch.ones_like(y, dtype=torch.bool)
    outside[:M, PAD:PAD + wc] = False
    if bool((y[outside] != SENT).any()):
        idx = ((y != SENT) & outside).nonzero()[0].tolist()
        fails.append(f"wrote outside the output window at buffer cell {idx} (M = {M}, columns {PAD}..{PAD + wc - 1})")
    body = y[:M, PAD:PAD + wc]
    if c.ref is not None:
        ne = body != c.ref[:, :wc]
        if bool(ne.any()):
            m, n = ne.nonzero()[0].tolist()
            fails.append(f"y[{m}, {n}] = {float(body[m, n])}, exact answer {float(c.ref[m, n])} "
                         f"({int(ne.sum())} of {ne.numel()} differ)")
    else:
        bad, worst = judge(body, c.r64, delta)
        if bool(bad.any()):
            m, n = bad.nonzero()[0].tolist()
            fails.append(f"y[{m}, {n}] = {float(body[m, n])}, float64 {float(c.r64[m, n])} "
                         f"({int(bad.sum())} of {bad.numel()} outside the allowance, worst ratio {worst:.3f})")
    for name, got, want in (("ss", ss, getattr(c, "ss_ref", None)), ("k_cache", kc, getattr(c, "kc_ref", None)),
                            ("v_cache", vc, getattr(c, "vc_ref", None)),
                            ("res_out", res_out, getattr(c, "res_out_ref", None))):
        if want is None:
            continue
        if got is None:
            fails.append(f"{name} missing")
        elif not torch.equal(got, want):
            idx = (got != want).nonzero()[0].tolist()
            fails.append(f"{name}{idx} = {float(got[tuple(idx)])}, exact answer {float(want[tuple(idx)])} "
                         f"({int((got != want).sum())} differ)")
    return fails, worst


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------

def _case(**kw):
    c = types.SimpleNamespace(ref=None, r64=None, bias64=None, sc64=None, splits_k=None)
    c.__dict__.update(kw)
    return c


def dense(M, N, K, seed, device="cpu", wscale=1.0):
    """epi 0: X ±1, W w_values(K) * wscale; Y = X W^T exactly."""
    g = _gen(seed)
    x = _pick((1.0, -1.0), (M, K), g).to(device)
    w = (_pick(w_values(K), (N, K), g) * wscale).to(device)
    y = x @ w.T
    return _case(kind="plain", M=M, N=N, K=K, cols=N, wcols=N, quantum=wscale, x=x.to(BF), w=w.to(BF), xin64=x,
                 w64=w, y64=y, ref=to_bf16(y))


def swiglu(M, I, K, seed, device="cpu", wscale=1.0, gshift=4):
    """epi 1: W = [gate * 2^-gshift; up]; |gate| <= 16; reference silu(g) u in float64."""
    c = dense(M, 2 * I, K, seed, device, wscale)
    c.w64[:I] *= 2.0 ** -gshift
    c.w = c.w64.to(BF)
    c.y64 = c.xin64 @ c.w64.T
    c.kind, c.I, c.cols, c.wcols, c.gshift, c.ref = "swiglu", I, I, I, gshift, None
    c.quantum = wscale * 2.0 ** -gshift
    c.r64 = silu_mul64(c.y64[:, :I], c.y64[:, I:])
    return c


def silu_mul64(g, u):
    return g / (1.0 + torch.exp(-g)) * u


def probe(M, N, K, device="cpu"):
    """x[m, k_m] = 1, k_m = (37 m + 5) % K; w[n, k] = ((131 n + 7 k) % 251) - 125: Y[m, n] = W[n, k_m]."""
    km = (37 * torch.arange(M) + 5) % K
    x = torch.zeros(M, K, dtype=torch.float64)
    x[torch.arange(M), km] = 1.0
    w = (((131 * torch.arange(N)[:, None] + 7 * torch.arange(K)[None, :]) % 251) - 125).double()
    x, w = x.to(device), w.to(device)
    y = w[:, km.to(device)].T.contiguous()
    return _case(kind="plain", M=M, N=N, K=K, cols=N, wcols=N, quantum=1.0, x=x.to(BF), w=w.to(BF), xin64=x, w64=w,
                 y64=y, ref=to_bf16(y), km=km)


def fold_probe(M, N, device="cpu", seed=77):
    """K = 512 in four 128-deep pieces.  The second 64 k of each piece carry W = ±2^-8, and pieces
    1 / 3 repeat the X and negate the W of pieces 0 / 2 there: every piece's partial has up to 16
    significant bits (a bf16-rounded piece loses them), the total is the integer of the first halves."""
    c = dense(M, N, 512, seed, device)
    g = _gen(seed + 1)
    lo = _pick((1.0, -1.0), (N, 2, 64), g).to(device) * 2.0 ** -8
    x, w = c.xin64, c.w64
    for p in (0, 2):
        a, b = 128 * p + 64, 128 * (p + 1) + 64
        w[:, a:a + 64] = lo[:, p // 2]
        w[:, b:b + 64] = -lo[:, p // 2]
        x[:, b:b + 64] = x[:, a:a + 64]
    c.x, c.w = x.to(BF), w.to(BF)
    c.y64 = x @ w.T
    c.ref = to_bf16(c.y64)
    c.quantum = 2.0 ** -8
    c.splits_k = 4
    return c


def residual(M, N, K, seed, device="cpu"):
    """EPI 2: Y <- Y + X W^T in place, ss[m, tile] = sum of the squares of the stored tile row."""
    c = dense(M, N, K, seed, device)
    g = _gen(seed + 1)
    old = (torch.randint(-60, 61, (M, N), generator=g).double() + 0.5 * (torch.randint(0, 4, (M, N), generator=g) == 0))
    c.y_old = old.to(device).to(BF)
    c.new64 = c.y_old.double() + c.y64
    c.kind, c.ref = "res", to_bf16(c.new64)
    c.ss_ref = (c.ref.double() ** 2).view(M, N // 256, 256).sum(-1).float()
    return c


def _pow2(e):
    """2^e in float64 for an integer tensor e, computed on the CPU (a device pow / exp2 / ldexp need
    not be exact) and moved to e's device."""
    ec = e.cpu().int()
    return torch.ldexp(torch.ones(ec.shape, dtype=torch.float64), ec).to(e.device)


def ss_rows(M, K, ss_ld, device="cpu"):
    """Row partials whose sum is K * 4^-j, j = m % 3, with every column in use; and j."""
    j = torch.arange(M) % 3
    ss = ((torch.arange(ss_ld).double() + 1) / 256).repeat(M, 1) + (K / 32 * 4.0 ** -j.double())[:, None]
    ss[:, 0] = 0
    ss[:, 0] = K * 4.0 ** -j.double() - ss.sum(-1)
    return ss.float().to(device), j.to(device)


def normed(M, N, K, kind, seed, device="cpu", ss_ld=8):
    """EPI 3 (kind 3) / EPI 4 (kind 4, N = 2 I rows of W): the accumulators times rstd = 2^j."""
    if kind == 4:
        c = swiglu(M, N // 2, K, seed, device, wscale=0.25, gshift=4)
    else:
        c = dense(M, N, K, seed, device, wscale=0.25)
    c.ss, c.j = ss_rows(M, K, ss_ld, device)
    c.sc64 = _pow2(c.j)[:, None]
    z = c.y64 * c.sc64
    if kind == 4:
        c.kind, c.r64 = "normswiglu", silu_mul64(z[:, :c.I], z[:, c.I:])
    else:
        c.kind, c.ref = "norm", to_bf16(z)
    c.z64 = z
    return c


def quarter_table(npos, device="cpu"):
    """cos_sin [npos, 128] = 64 cos | 64 sin of quarter turns t(p, i) = (p + 3 i + (i >> 4)) % 4."""
    p, i = torch.arange(npos)[:, None], torch.arange(64)[None, :]
    t = (p + 3 * i + (i >> 4)) % 4
    cos = torch.tensor([1.0, 0.0, -1.0, 0.0])[t]
    sin = torch.tensor([0.0, 1.0, 0.0, -1.0])[t]
    return torch.cat([cos, sin], 1).contiguous().to(device)


def rotate(h, cs, partner=64, sin_sign=1.0):
    """NeoX rotation of h [M, H, 128] by cs [M, 128]: (d, d + 64) pairs; the slips pair d with d + 32
    or flip the sine."""
    c, s = cs[:, None, :64].double(), sin_sign * cs[:, None, 64:].double()
    x0, x1 = h[..., :64], h[..., 64:]
    xp = x1 if partner == 64 else torch.roll(h, -partner, -1)[..., :64]
    return torch.cat([x0 * c - xp * s, x1 * c + x0 * s], -1)


NPOS, BS, NB = 64, 16, 32          # RoPE table rows; page size and pages of the test caches (512 slots)


def rope_io(M, device="cpu"):
    """positions, slots (distinct; -1 at both ends of a row tile and at the last row when M > 1)."""
    m = torch.arange(M)
    pos = ((5 * m + 1) % NPOS).int()
    slots = ((7 * m + 3) % (NB * BS)).int()
    if M > 1:
        for r in (0, 255, 256, M - 1):
            if r < M:
                slots[r] = -1
    return pos.to(device), slots.to(device)


def rope_expect(z64, pos, slots, table, nh, nkv, fused, partner=64, sin_sign=1.0):
    """From the (normalised) qkv z64 [M, (nh + 2 nkv) 128]: the Y window, k cache and v cache (bf16,
    SENT where nothing is written).  fused: Y keeps the raw k / v columns (fused_decode.hip); else they
    are not written (mfma_gemm.hip EPI 5)."""
    M, dev = z64.shape[0], z64.device
    cs = table[pos.long()]
    q = rotate(z64[:, :nh * 128].view(M, nh, 128), cs, partner, sin_sign)
    k = rotate(z64[:, nh * 128:(nh + nkv) * 128].view(M, nkv, 128), cs, partner, sin_sign)
    v = z64[:, (nh + nkv) * 128:].view(M, nkv, 128)
    y = torch.cat([q.reshape(M, -1), z64[:, nh * 128:]], 1) if fused else q.reshape(M, -1)
    kc = torch.full((NB, nkv, BS, 128), SENT, dtype=BF, device=dev)
    vc = torch.full((NB, nkv, BS, 128), SENT, dtype=BF, device=dev)
    live = slots >= 0
    s = slots[live].long()
    kc[s // BS, :, s % BS] = to_bf16(k[live])
    vc[s // BS, :, s % BS] = to_bf16(v[live])
    return to_bf16(y), kc, vc


def normed_rope(M, nh, nkv, K, seed, device="cpu", ss_ld=8):
    """EPI 5: the normalised qkv projection with quarter-turn RoPE and the paged-KV write."""
    c = normed(M, (nh + 2 * nkv) * 128, K, 3, seed, device, ss_ld)
    c.kind, c.nh, c.nkv = "rope", nh, nkv
    c.pos, c.slots = rope_io(M, device)
    c.table = quarter_table(NPOS, device)
    c.ref, c.kc_ref, c.vc_ref = rope_expect(c.z64, c.pos, c.slots, c.table, nh, nkv, False)
    c.wcols = nh * 128
    return c


def gains(K):
    """RMSNorm gains in {0.5, 1, 2}: 2 at k % 32 == 0, 1 at k % 32 in 1..3, 0.5 elsewhere (keeps the
    half-integer outputs of a dense K = 1024 row below 128, where bf16 still holds them)."""
    k = torch.arange(K) % 32
    return torch.where(k == 0, 2.0, torch.where(k < 4, 1.0, 0.5)).double()


def fused(M, R, K, pro, epi, seed, device="cpu", nh=0, nkv=0, sparse=False):
    """fused_skinny: pro 0 X ±1; pro 1 X ±2 (rstd = 1/2, eps 0) with ``gains``; pro 2 the same sum
    from x in {±1, ±3} plus a residual.  W ±1 (gate rows * 2^-4 for epi 1).  Integer bias on every row
    but the gate rows, which get multiples of 1/2 in [-1, 1].  sparse: each X row nonzero on a quarter
    of the k (k % 4 == m % 4; pro >= 1: ±4 there), for K too large for dense rows.
    Carries both answers: c.nobias and c.withbias hold (ref, r64)."""
    g = _gen(seed)
    sgn = _pick((1.0, -1.0), (M, K), g)
    keep = torch.ones(M, K)
    amp = 2.0
    if sparse:
        keep = ((torch.arange(K)[None, :] % 4) == (torch.arange(M)[:, None] % 4)).double()
        amp = 4.0
    c = _case(kind=("fused0", "fused1", "fused2")[epi], M=M, N=R, K=K, pro=pro, epi=epi, nh=nh, nkv=nkv,
              quantum=2.0 ** -5 if epi == 1 else 0.5, res=None, gamma=None, res_out_ref=None, sparse=sparse)
    if pro == 0:
        hsum = sgn * keep
        c.x = hsum.to(device).to(BF)
        xin = hsum
    else:
        hsum = amp * sgn * keep
        c.gamma = gains(K).to(device).to(BF)
        if pro == 2:
            xx = _pick((1.0, -1.0, 3.0, -3.0), (M, K), g) * keep
            c.x, c.res = xx.to(device).to(BF), (hsum - xx).to(device).to(BF)
            c.res_out_ref = hsum.to(device).to(BF)
        else:
            c.x = hsum.to(device).to(BF)
        assert bool(((hsum ** 2).sum(-1) == 4 * K).all())            # rstd = 1/2 exactly
        xin = hsum * 0.5 * gains(K)[None, :]
    w = _pick((1.0, -1.0), (R, K), g)
    bias = torch.randint(-8, 9, (R,), generator=g).double()
    if epi == 1:
        I = R // 2
        w[:I] *= 2.0 ** -4
        bias[:I] = torch.randint(-2, 3, (I,), generator=g).double() / 2
        c.I = I
    c.xin64, c.w64, c.bias64 = xin.to(device), w.to(device), bias.to(device)
    c.w, c.bias = c.w64.to(BF), c.bias64.to(BF)
    c.y64 = c.xin64 @ c.w64.T
    c.cols = c.wcols = R // 2 if epi == 1 else R
    if epi == 2:
        c.pos, c.slots = rope_io(M, device)
        c.table = quarter_table(NPOS, device)
    c.nobias, c.withbias = _fused_answer(c, c.y64), _fused_answer(c, c.y64 + c.bias64[None, :])
    return c


def _fused_answer(c, z):
    a = types.SimpleNamespace(ref=None, r64=None, kc_ref=None, vc_ref=None, z64=z)
    if c.epi == 0:
        a.ref = to_bf16(z)
    elif c.epi == 1:
        a.r64 = silu_mul64(z[:, :c.I], z[:, c.I:])
    else:
        a.ref, a.kc_ref, a.vc_ref = rope_expect(z, c.pos, c.slots, c.table, c.nh, c.nkv, True)
    return a


def with_answer(c, a):
    """Case c judged against one of its answers (fused cases carry two)."""
    d = types.SimpleNamespace(**c.__dict__)
    d.__dict__.update(a.__dict__)
    return d


def check(c):
    """The conditions that make case c's answer exact; raises AssertionError naming the one missed."""
    q = c.quantum
    zs = [c.y64] + [a.z64 for a in (getattr(c, "nobias", None), getattr(c, "withbias", None)) if a is not None]
    if c.sc64 is not None:
        zs.append(c.z64)
    for z in zs:
        assert torch.equal(z / q, (z / q).round()), "a sum is no multiple of the case's quantum"
        assert float(z.abs().max()) / q < 2 ** 24, "a sum does not fit fp32"
    # partial sums over any subset are bounded by sum |x| |w|
    assert float((c.xin64.abs() @ c.w64.abs().T).max()) / q < 2 ** 24, "a partial sum may not fit fp32"
    assert is_bf16(c.xin64) and is_bf16(c.w64), "operands are not bf16"
    assert hasattr(c, "km") or bool((c.w64 != 0).all()), "a zero weight"
    if c.kind in ("plain", "res", "norm", "rope", "fused0", "fused2"):
        for z in zs:
            assert is_bf16(z), "a final value is not representable in bf16"
            assert float(z.abs().max()) <= 256, "|y| > 256"
    if c.kind in ("swiglu", "normswiglu", "fused1"):
        for z in zs[-1:] if c.sc64 is not None else zs:
            assert is_bf16(z), "gate / up are not representable in bf16"
            assert float(z[:, :c.I].abs().max()) <= 16, "|gate| > 16"
    if c.kind == "res":
        assert float(c.new64.abs().max()) < 256, "|Y_new| >= 256"
        assert torch.equal(c.new64 * 2, (c.new64 * 2).round())
        assert c.new64.numel() < 25600 or bool((c.ref.double() != c.new64).any()), "no stored value was rounded"
        assert float(c.ss_ref.max()) * 4 < 2 ** 24, "4 ss >= 2^24"
    if c.sc64 is not None:
        s32 = c.ss.sum(-1)                                           # exact: multiples of 2^-8 below 2^13
        assert torch.equal(s32.double(), c.ss.double().sum(-1))
        inv_k = torch.tensor(1.0 / c.K, dtype=torch.float32, device=s32.device)
        assert torch.equal((s32 * inv_k).double(), _pow2(-2 * c.j)), "ss / K is no power of four in fp32"
        assert bool((c.ss != 0).all()) and float(c.ss.max()) < 2 ** 24
    if getattr(c, "sparse", False):
        assert bool((c.xin64 != 0).any(0).all()), "a k that is zero in every row"
    elif not hasattr(c, "km"):
        assert bool((c.xin64 != 0).all()), "a zero activation"
    return c


# ---------------------------------------------------------------------------------------------
# the launch plan of the ping-pong kernel
# ---------------------------------------------------------------------------------------------

def pp_plan(M, N, K, swiglu, streamk, overlap, P):
    """The decomposition ``launch_pp`` picks (mfma_gemm.hip): N rows of W, streamk 0 auto / 1 off /
    2 whenever it applies, P the CU count rounded down to a multiple of 8.  Returns a dict: tiles,
    grid, persistent, rem (tiles cut along K), splits (pieces per cut tile), full (whole tiles per
    block of a persistent launch)."""
    tiles_m = (M + 255) // 256
    tiles = tiles_m * (N // 2 // 128 if swiglu else N // 256)
    plan = dict(tiles=tiles, grid=tiles, persistent=False, rem=0, splits=0, full=0)
    skmode = {0: 1, 1: 0, 2: 2}[streamk]
    if (skmode or overlap) and K // 64 >= 8:
        full, rem = divmod(tiles, P)
        splits = min(4, P // rem) if rem else 0
        if skmode and splits >= 2 and (full < 8 or skmode == 2):
            plan.update(grid=P, persistent=True, rem=rem, splits=splits, full=full)
        elif overlap and rem == 0 and full >= 2:
            plan.update(grid=P, persistent=True, full=full)
    return plan


def pieces(K, splits):
    """K ranges of the pieces of a cut tile (128-deep units, as in ``drive``)."""
    u = K // 128
    if splits == 1:
        return [(0, K)]
    return [(128 * (j * u // splits), 128 * ((j + 1) * u // splits)) for j in range(splits)]


def n_for(want, M, N, K, P, streamk=0, overlap=True):
    """N (rows of W, epi 0) at which (M, N, K) reaches the plan ``want`` (a subset of pp_plan's keys)
    on a device of P CUs: the given N if it does (P = 256), else the smallest multiple of 256."""
    def hit(n):
        p = pp_plan(M, n, K, False, streamk, overlap, P)
        return all(p[k] == v for k, v in want.items())
    if hit(N):
        return N
    for n in range(256, 256 * 129, 256):
        if hit(n):
            return n
    raise AssertionError(f"no N reaches {want} at M = {M}, K = {K}, P = {P}")


# ---------------------------------------------------------------------------------------------
# a CPU model of the kernels, with one switchable slip each
# ---------------------------------------------------------------------------------------------

def _store(v64, mutate):
    if mutate == "truncate":
        return (v64.float().view(torch.int32) & -65536).view(torch.float32).to(BF)
    return to_bf16(v64)


def kernel_model(c, mutate=None, splits=None, bias=False):
    """What the kernel of case c's family computes, as a dict of ``verdict``'s arguments; ``mutate``
    (one of MUTATIONS) switches one slip on.  splits: pieces of the K split (default: c.splits_k or 1)."""
    assert mutate is None or mutate in MUTATIONS
    x, w = c.xin64.clone(), c.w64
    M, K = x.shape
    if mutate == "drop_k":
        x[M - 1, (K // 3) | 1] = 0
    if mutate == "swap_chunks":
        r = M // 2
        a = (37 * r + 5) % K // 8 * 8                 # the chunk a probe's row r is hot in
        b = a ^ 16
        x[r, a:a + 8], x[r, b:b + 8] = x[r, b:b + 8].clone(), x[r, a:a + 8].clone()
    splits = splits or c.splits_k or 1
    parts = [x[:, a:b] @ w[:, a:b].T for a, b in pieces(K, splits)]
    if mutate == "round_piece":
        parts[1] = to_bf16(parts[1]).double()
    if mutate == "skip_piece":
        parts = parts[:-1]
    acc = sum(parts)
    if bias:
        acc = acc + c.bias64[None, :]
    out = {}
    if c.sc64 is not None:
        ss = c.ss[:, :-1] if mutate == "short_ss" else c.ss
        acc = acc * torch.rsqrt(ss.double().sum(-1) / K)[:, None]
    if c.kind in ("swiglu", "normswiglu", "fused1"):
        g, u = acc[:, :c.I], acc[:, c.I:]
        if mutate == "swap_gate_up":
            g, u = u, g
        val = _store(silu_mul64(g, u), mutate)
    elif c.kind == "res":
        new = c.y_old.double() + acc
        val = _store(new, mutate)
        src = new if mutate == "ss_fp32" else val.double()
        out["ss"] = (src ** 2).view(M, c.N // 256, 256).sum(-1).float()
    elif c.kind in ("rope", "fused2"):
        z = _store(acc, mutate).double()
        val, out["kc"], out["vc"] = rope_expect(z, c.pos, c.slots, c.table, c.nh, c.nkv, c.kind == "fused2",
                                                partner=32 if mutate == "partner32" else 64,
                                                sin_sign=-1.0 if mutate == "sin_sign" else 1.0)
        val = val[:, :c.wcols]
    else:
        val = _store(acc, mutate)
    y = torch.full((M + TAIL, c.wcols + 2 * PAD), SENT, dtype=BF, device=val.device)
    y[:M, PAD:PAD + c.wcols] = val
    if mutate == "row_past_m":
        y[M, PAD:PAD + c.wcols] = val[M - 1]
    out["y"] = y
    if getattr(c, "res_out_ref", None) is not None:
        out["res_out"] = c.res_out_ref.clone()
    return out


def swiglu_cpu_cases():
    """The neighbour-rule cases small enough for the CPU tests; FP32_GAP is measured over them."""
    yield "swiglu 129x128x256", check(swiglu(129, 128, 256, 11))
    yield "swiglu 200x128x512", check(swiglu(200, 128, 512, 12))
    yield "swiglu 64x128x1152", check(swiglu(64, 128, 1152, 13))
    yield "normswiglu 100x256x256", check(normed(100, 512, 256, 4, 14))
    yield "normswiglu 257x256x512", check(normed(257, 512, 512, 4, 15, ss_ld=32))
    for pro in (0, 1, 2):
        c = check(fused(16, 64, 1024, pro, 1, 16 + pro))
        yield f"fused pro {pro} epi 1 16x32x1024", with_answer(c, c.withbias)


def gate_up(c):
    """The exact (gate, up) of a neighbour-rule case."""
    z = c.z64 if getattr(c, "z64", None) is not None else c.y64
    return z[:, :c.I], z[:, c.I:]
