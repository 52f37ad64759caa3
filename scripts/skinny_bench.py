#!/usr/bin/env python3
"""Decode-sized GEMMs: hipBLASLt (F.linear) vs the weight-streaming skinny kernel.

Weights rotate over enough copies (> 1 GiB) that every call streams from HBM,
as in a real decode step where a layer's weights were last touched one full
model pass ago (the 256 MB MALL cannot hold them).  Prints one JSON line per
(shape, M, impl) with the time and the achieved weight bandwidth.  ``--fp8-cfg``
adds the W8A16 kernel (``skinny_gemm_w8``, e4m3 weights at half the bytes) as
``fp8_c<cfg>`` columns, over the same number of rotating copies; ``--w4-cfg`` the
W4A16 kernel (``skinny_gemm_w4``, MXFP4 weights at a quarter of the bytes plus one scale
byte per 32 elements) as ``w4_c<cfg>``.  ``-1`` in either list stands for the config the
ops layer picks for the shape and row count.
"""
import argparse
import json
import sys
import os

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dgi import ops  # noqa: E402

SHAPES = {  # name: (N, K)
    "8b_qkv": (6144, 4096), "8b_o": (4096, 4096), "8b_gate_up": (28672, 4096), "8b_down": (4096, 14336),
    "lm_head": (128256, 4096),
    "70b_qkv": (10240, 8192), "70b_o": (8192, 8192), "70b_gate_up": (57344, 8192), "70b_down": (8192, 28672),
}


def timed(fn, iters, graph=False, reps=5):
    for _ in range(3):
        fn(0)
    torch.cuda.synchronize()
    if graph:
        # one captured graph of ``iters`` launches over the rotating copies, replayed ``reps`` times:
        # kernel time without the host's launch gaps (short kernels are launch-bound eagerly)
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                for i in range(iters):
                    fn(i)
        g.replay()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / (iters * reps) * 1000.0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ms", type=int, nargs="+", default=[1, 2, 4, 8, 16, 32])
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES))
    ap.add_argument("--cfg", type=int, nargs="+", default=[0], choices=[0, *sorted(ops.SKINNY_CFGS)])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--fp8-cfg", type=int, nargs="*", default=[0], help="skinny_gemm_w8 launch configs (none: skip)")
    ap.add_argument("--w4-cfg", type=int, nargs="*", default=[], help="skinny_gemm_w4 launch configs (none: skip)")
    ap.add_argument("--no-hipblaslt", action="store_true")
    ap.add_argument("--graph", action="store_true", help="time hipGraph replays instead of eager launches")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ops.load_native(required=True)
    rows = []
    for name in a.shapes:
        N, K = SHAPES[name]
        copies = max(2, -(-(1 << 30) // (N * K * 2)))
        ws = [torch.randn(N, K, device="cuda", dtype=torch.bfloat16) * 0.02 for _ in range(copies)]
        qs = [ops.quantize_fp8(w) for w in ws] if a.fp8_cfg else []
        q4 = [ops.quantize_mxfp4(w) for w in ws] if a.w4_cfg else []
        for M in a.ms:
            x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
            out = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
            impls = {} if a.no_hipblaslt else {"hipblaslt": lambda i: F.linear(x, ws[i % copies])}
            for c in a.cfg:
                impls[f"skinny_c{c}"] = (lambda c_: lambda i: torch.ops.dgi.skinny_gemm(
                    out, x, ws[i % copies], None, c_))(c)
            for c in a.fp8_cfg:
                pick = ops._skinny_w8_cfg(M, N) if c < 0 else c
                if ops.skinny_w8_cfg_ok(pick, N, K):
                    impls["fp8_pick" if c < 0 else f"fp8_c{c}"] = (lambda c_: lambda i: torch.ops.dgi.skinny_gemm_w8(
                        out, x, qs[i % copies].q, qs[i % copies].scale, None, c_))(pick)
            for c in a.w4_cfg:
                pick = ops._skinny_w4_cfg(M, N, K) if c < 0 else c
                if ops.skinny_w4_cfg_ok(pick, N, K):
                    impls["w4_pick" if c < 0 else f"w4_c{c}"] = (lambda c_: lambda i: torch.ops.dgi.skinny_gemm_w4(
                        out, x, q4[i % copies].q, q4[i % copies].scale, None, c_))(pick)
            ref = F.linear(x.float(), ws[0].float())
            torch.ops.dgi.skinny_gemm(out, x, ws[0], None, 0)
            err = (out.float() - ref).abs().max().item()
            err8 = None
            if a.fp8_cfg:
                torch.ops.dgi.skinny_gemm_w8(out, x, qs[0].q, qs[0].scale, None, 0)
                err8 = (out.float() - F.linear(x.float(), qs[0].dequant())).abs().max().item()
            err4 = rms4 = None
            if a.w4_cfg:
                torch.ops.dgi.skinny_gemm_w4(out, x, q4[0].q, q4[0].scale, None, 0)
                err4 = (out.float() - F.linear(x.float(), q4[0].dequant())).abs().max().item()
                # what the format costs: the quantised projection against the bf16 one, relative rms
                rms4 = ((out.float() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()
            for impl, fn in impls.items():
                us = timed(fn, a.iters, a.graph)
                fp8, w4 = impl.startswith("fp8"), impl.startswith("w4")
                nbytes = N * K * 2 if not (fp8 or w4) else qs[0].nbytes() if fp8 else q4[0].nbytes()
                rows.append({"shape": name, "M": M, "N": N, "K": K, "impl": impl, "us": round(us, 2),
                             "weight_TBs": round(nbytes / us / 1e6, 2),
                             "max_err": round(err8 if fp8 else err4 if w4 else err, 4),
                             "timing": "graph" if a.graph else "eager"})
                if w4:
                    rows[-1]["rel_rms_vs_bf16"] = round(rms4, 4)
                if impl.endswith("_pick"):
                    rows[-1]["cfg"] = ops._skinny_w8_cfg(M, N) if fp8 else ops._skinny_w4_cfg(M, N, K)
                print(json.dumps(rows[-1]), flush=True)
        del ws, qs, q4
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
