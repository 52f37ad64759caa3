"""Bandwidth of the memory-bound dgi kernels (silu_mul, fused_add_rmsnorm, rmsnorm) at serving shapes."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from dgi import ops


def timed(fn, iters=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


for T in (64, 384, 1920, 4096):
    I, H = 28672, 8192
    gu = torch.randn(T, 2 * I, device="cuda", dtype=torch.bfloat16)
    out = torch.empty(T, I, device="cuda", dtype=torch.bfloat16)
    us = timed(lambda: ops.silu_mul(gu, out=out))
    print(json.dumps({"kernel": "silu_mul", "T": T, "I": I, "us": round(us, 2), "TBs": round(3 * T * I * 2 / us / 1e6, 2)}))
    x = torch.randn(T, H, device="cuda", dtype=torch.bfloat16)
    r = torch.randn(T, H, device="cuda", dtype=torch.bfloat16)
    w = torch.randn(H, device="cuda", dtype=torch.bfloat16)
    us = timed(lambda: ops.fused_add_rmsnorm(x, r, w, 1e-5))
    print(json.dumps({"kernel": "fused_add_rmsnorm", "T": T, "H": H, "us": round(us, 2), "TBs": round(4 * T * H * 2 / us / 1e6, 2)}))
    us = timed(lambda: ops.rmsnorm(x, w, 1e-5))
    print(json.dumps({"kernel": "rmsnorm", "T": T, "H": H, "us": round(us, 2), "TBs": round(2 * T * H * 2 / us / 1e6, 2)}), flush=True)

# the RoPE + paged-KV writers: rope_cache and its q/k-norm variant (Qwen3) move the same bytes —
# the qkv row read once, q written back, k and v written to the pages (2 bytes per element, or 1 for
# e4m3 pages).  Llama-3-8B / Qwen3-8B heads (32 / 8) and Qwen3-32B heads (64 / 8), head_dim 128.
BS = 16
for nh, nkv, hd in ((32, 8, 128), (64, 8, 128)):
    cs = ops.rope_cos_sin(hd, 8192, 1e6, device="cuda")
    qg = (0.25 + 3.75 * torch.rand(hd, device="cuda")).bfloat16()
    kg = (0.25 + 3.75 * torch.rand(hd, device="cuda")).bfloat16()
    for T in (1, 16, 512, 4096):
        qkv = torch.randn(T, (nh + 2 * nkv) * hd, device="cuda", dtype=torch.bfloat16)
        pos = torch.randint(0, 8192, (T,), device="cuda", dtype=torch.int32)
        nblk = (T + BS - 1) // BS
        slots = torch.randperm(nblk * BS, device="cuda")[:T].to(torch.int32)
        for pages in ("bf16", "fp8"):
            kv = torch.zeros(2, nblk, nkv, BS, hd, device="cuda",
                             dtype=torch.bfloat16 if pages == "bf16" else ops.KV_FP8)
            inv = torch.ones(2, nkv, device="cuda") if pages == "fp8" else None
            byts = T * hd * ((nh + 2 * nkv) * 2 + nh * 2 + 2 * nkv * kv.element_size())
            us = {"rope_cache": timed(lambda: ops.rope_cache(qkv, pos, cs, nh, nkv, hd, slots, kv[0], kv[1], 0,
                                                             kv_inv_scale=inv), iters=200),
                  "qknorm_rope_cache": timed(lambda: ops.qknorm_rope_cache(qkv, pos, cs, qg, kg, 1e-6, nh, nkv, hd, slots,
                                                                           kv[0], kv[1], kv_inv_scale=inv), iters=200)}
            for k, v in us.items():
                print(json.dumps({"kernel": k, "nh": nh, "nkv": nkv, "hd": hd, "T": T, "pages": pages, "us": round(v, 2),
                                  "TBs": round(byts / v / 1e6, 3),
                                  "vs_rope_cache": round(v / us["rope_cache"], 3)}), flush=True)
