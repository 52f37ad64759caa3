#!/usr/bin/env python3
"""Prefill-sized projections of an fp8 weight: the W8A8 kernels against the routes they replace.

Per (shape, M), hipGraph-timed as in ``skinny_bench.py --graph`` with the weights rotating over
enough copies that every call streams them from HBM:

  a  ``dequant_fp8`` + the bf16 GEMM (``F.linear``): the route of an fp8 weight without ``act="fp8"``
  b  the bf16 GEMM on bf16 weights: ``F.linear`` (b_hipblaslt) and ``ops.mfma_gemm`` (b_mfma)
  c  ``quant_rows_fp8`` + ``mfma_gemm_fp8``: the W8A8 route
  d  ``mfma_gemm_fp8`` alone
  d1 ``mfma_gemm`` simple kernel (sched 1): the bf16 kernel the e4m3 one is modelled on

Prints one JSON line per (shape, M, impl); ``--check`` also prints the W8A8 result's relative rms
error against the bf16 product.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dgi import ops  # noqa: E402
from skinny_bench import SHAPES, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ms", type=int, nargs="+", default=[64, 256, 512, 1024, 2048, 4096])
    ap.add_argument("--shapes", nargs="+", default=[s for s in SHAPES if s != "lm_head"])
    ap.add_argument("--impls", nargs="+", default=["a", "b_hipblaslt", "b_mfma", "c", "d", "d1"])
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ops.load_native(required=True)
    rows = []
    for name in a.shapes:
        N, K = SHAPES[name]
        # > 1 GiB of e4m3 copies (four times the 256 MB cache), and every graph walks all of them, so
        # neither the fp8 nor the (twice as large) bf16 routes find a weight in cache
        copies = max(2, -(-(1 << 30) // (N * K)))
        iters = max(a.iters, copies)
        ws = [torch.randn(N, K, device="cuda", dtype=torch.bfloat16) * 0.02 for _ in range(copies)]
        qs = [ops.quantize_fp8(w) for w in ws]
        scratch = torch.empty(N * K, device="cuda", dtype=torch.bfloat16)
        for M in a.ms:
            x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
            out = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
            xq, sx = ops.quant_rows_fp8(x)

            def w8a8(i):
                torch.ops.dgi.quant_rows_fp8(xq, sx, x)
                torch.ops.dgi.mfma_gemm_fp8(out, xq, sx, qs[i % copies].q, qs[i % copies].scale, None)
            impls = {
                "a": lambda i: F.linear(x, ops.dequant_fp8(qs[i % copies], scratch)),
                "b_hipblaslt": lambda i: F.linear(x, ws[i % copies]),
                "b_mfma": lambda i: ops.mfma_gemm(x, ws[i % copies], 0, out),
                "c": w8a8,
                "d": lambda i: torch.ops.dgi.mfma_gemm_fp8(out, xq, sx, qs[i % copies].q, qs[i % copies].scale, None),
                "d1": lambda i: ops.mfma_gemm(x, ws[i % copies], 0, out, sched=1),
            }
            err = None
            if a.check:
                w8a8(0)
                ref = F.linear(x, ws[0]).float()
                err = float((out.float() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
            for impl in a.impls:
                us = timed(impls[impl], iters, graph=True, reps=a.reps)
                rows.append({"shape": name, "M": M, "N": N, "K": K, "impl": impl, "us": round(us, 1),
                             "TFLOPs": round(2.0 * M * N * K / us / 1e6, 1)})
                if err is not None and impl == "c":
                    rows[-1]["rel_rms_vs_bf16"] = round(err, 5)
                print(json.dumps(rows[-1]), flush=True)
        del ws, qs, scratch
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
