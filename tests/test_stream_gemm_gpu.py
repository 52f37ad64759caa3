"""The three dense weight-streaming GEMMs (skinny_gemm, skinny_gemm_w8, skinny_gemm_w4) against an
exact answer, over every launch config of each table.

Inputs are chosen so that every intermediate sum is exact: X is integers in [-4, 4], W is an e2m1
value (0, ±0.5, ... ±6) times 2^s with s in {-1, 0, 1}, the bias integers in [-8, 8].  Every partial
and total is a multiple of 2^-2 below 4 · 12 · 2048 + 8 < 2^17, 19 significant bits: exact in fp32 in
any summation order, so the only rounding is the final bf16 one and the fp64 reference (fp64 ->
fp32 exactly -> bf16) must be met bit for bit by every kernel, config, ring depth and row tile.

The same W is exact in bf16, as e4m3 codes with scale[n] = 2^s per row, and as mxfp4 with every
block scale of row n = 127 + s: the three formats hold one matrix.  A second case varies s per
32-element block, which only mxfp4 can hold; it pins each scale byte to its block."""
import pytest
import torch

from dgi import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, K = 128, 2048            # the smallest K every config of the three tables divides; two workgroups at four column tiles
MS = (1, 16, 17, 32)        # the edges of both row tiles
E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


@pytest.fixture(autouse=True, scope="module")
def _native():
    ops.load_native(required=True)


def _case(per_block: bool):
    """X [32, K], bias [N], the weight in fp64 and in each format that holds it, and the fp64 answer."""
    g = torch.Generator(device="cpu").manual_seed(20 + per_block)
    codes = torch.randint(0, 16, (N, K), generator=g)
    s = torch.randint(-1, 2, (N, K // 32) if per_block else (N, 1), generator=g).expand(N, K // 32).contiguous()
    table = torch.tensor(E2M1 + tuple(-v for v in E2M1), dtype=torch.float64)
    w64 = (table[codes].view(N, K // 32, 32) * torch.exp2(s.double())[:, :, None]).view(N, K).to(DEV)
    fmts = {"w4": ((codes[:, 0::2] | (codes[:, 1::2] << 4)).to(torch.uint8).contiguous().to(DEV),
                   (127 + s).to(torch.uint8).to(DEV))}
    if not per_block:
        wb = w64.to(torch.bfloat16)
        q8 = table[codes].float().to(torch.float8_e4m3fn).to(DEV)
        sc8 = torch.exp2(s[:, 0].float()).to(DEV)
        assert torch.equal(wb.double(), w64) and torch.equal(q8.float().double() * sc8.double()[:, None], w64)
        fmts["bf16"] = (wb,)
        fmts["w8"] = (q8, sc8)
    x = torch.randint(-4, 5, (32, K), generator=g).to(torch.bfloat16).to(DEV)
    bias = torch.randint(-8, 9, (N,), generator=g).to(torch.bfloat16).to(DEV)
    y64 = x.double() @ w64.T
    assert y64.abs().max() + 8 < 2 ** 17 and torch.equal(y64 * 4, (y64 * 4).round())
    refs = {False: y64.float().to(torch.bfloat16), True: (y64 + bias.double()).float().to(torch.bfloat16)}
    return x, bias, fmts, refs


# op, config table, whether a config divides [N, K]
KERNELS = {"bf16": ("skinny_gemm", ops.SKINNY_CFGS, lambda cfg: ops._skinny_cfg_ok(ops.SKINNY_CFGS, 4, 64, cfg, N, K)),
           "w8": ("skinny_gemm_w8", ops.SKINNY_W8_CFGS, lambda cfg: ops.skinny_w8_cfg_ok(cfg, N, K)),
           "w4": ("skinny_gemm_w4", ops.SKINNY_W4_CFGS, lambda cfg: ops.skinny_w4_cfg_ok(cfg, N, K))}


@pytest.mark.parametrize("per_block", [False, True], ids=["row_scales", "block_scales"])
def test_stream_gemm_exact(per_block):
    x32, bias, fmts, refs = _case(per_block)
    ran = skipped = 0
    for fmt, weight in fmts.items():
        op, table, cfg_ok = KERNELS[fmt]
        for cfg in [0] + sorted(table):
            if not cfg_ok(cfg):
                skipped += 1
                continue
            for M in MS:
                x = x32[:M]         # rows M.. of the buffer are not zero: the kernel must not use them
                for wb in (False, True):
                    buf = torch.full((32, N), -77.0, dtype=torch.bfloat16, device=DEV)
                    getattr(torch.ops.dgi, op)(buf[:M], x, *weight, bias if wb else None, cfg)
                    assert torch.equal(buf[:M], refs[wb][:M]), f"{op} cfg {cfg} M {M} bias {wb}"
                    assert (buf[M:] == -77.0).all(), f"{op} cfg {cfg} M {M}: wrote rows past M"
                    ran += 1
    assert skipped == 0                      # K = 2048, N = 128 divide every geometry
    assert ran == sum(1 + len(KERNELS[f][1]) for f in fmts) * len(MS) * 2
