#!/usr/bin/env python3
"""MoE block timings on one GPU: the four kernels of dgi/csrc/moe.hip, ``ops.moe_mlp`` and the
per-expert torch loop (``ops.moe_mlp_ref`` on the GPU) on one layer's shapes (default
Qwen3-30B-A3B: H 2048, 128 experts of width 768, 8 per token).

Every timed piece is captured into one hipGraph that walks ``--layers`` independent copies of the
layer's weights (different routing per copy), so a replay streams each copy's experts from HBM as
a real model's layer loop does instead of re-reading one layer from the caches; times are per
layer, from device events around ``--reps`` replays.  The torch loop reads its routing back on the
host, cannot be captured, and is timed with a host clock around a synchronise.

For each T the distinct expert bytes a layer's two grouped GEMMs must stream (experts that got at
least one token) over their time is printed next to what ``skinny_gemm`` streams on a dense
[N, H] projection of the same byte count (M = min(T, 32) rows) in the same run.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dgi import ops  # noqa: E402


def graph_ms(fn, layers: int, reps: int) -> float:
    """ms per layer of ``fn(l)`` for l in range(layers), captured once and replayed ``reps`` times."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for l in range(layers):
            fn(l)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = [fn(l) for l in range(layers)]
    for _ in range(2):
        g.replay()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    del keep
    return a.elapsed_time(b) / (reps * layers)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, default=2048)
    ap.add_argument("--inter", type=int, default=768)
    ap.add_argument("--experts", type=int, default=128)
    ap.add_argument("--topk", type=int, default=8)
    ap.add_argument("--tokens", type=int, nargs="+", default=[1, 4, 16, 64, 512, 2048])
    ap.add_argument("--layers", type=int, default=6, help="independent weight copies a replay walks")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="write the JSON rows here as well")
    ap.add_argument("--expert-quant", default=None, choices=["fp8"],
                    help="also time the block and both grouped GEMMs over FP8 weight-only experts "
                         "(ops.quantize_fp8_experts of the same weights), beside the bf16 ones")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("moe_bench: needs a GPU")
    ops.load_native(required=True)
    dev = "cuda"
    H, I, E, k, L = a.hidden, a.inter, a.experts, a.topk, a.layers
    g = torch.Generator(device=dev).manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev)     # noqa: E731
    router = [(rn(E, H) / H ** 0.5).bfloat16() for _ in range(L)]
    gate_up = [(rn(E, 2 * I, H) / H ** 0.5).bfloat16() for _ in range(L)]
    down = [(rn(E, H, I) / I ** 0.5).bfloat16() for _ in range(L)]
    expert_bytes = 3 * H * I * 2
    gate_up_q = down_q = None
    if a.expert_quant == "fp8":
        gate_up_q = [ops.quantize_fp8_experts(w) for w in gate_up]
        down_q = [ops.quantize_fp8_experts(w) for w in down]
        expert_bytes_q = 3 * H * I + 4 * (2 * I + H)      # codes + one fp32 scale per output channel
    rows = []
    for T in a.tokens:
        x = [rn(T, H).bfloat16() for _ in range(L)]
        BM = ops.moe_block_rows(T, k, E)
        logits = [ops.linear(x[l], router[l]) for l in range(L)]
        routed = [ops.moe_route(logits[l], k, True) for l in range(L)]
        lay = [ops.moe_align(routed[l][0], E, BM) for l in range(L)]
        act = [ops.moe_gemm(x[l], gate_up[l], lay[l][2], lay[l][3], k, ops.MOE_EPI_SWIGLU, BM) for l in range(L)]
        y = [ops.moe_gemm(act[l], down[l], lay[l][2], lay[l][3], k, ops.MOE_EPI_PLAIN, BM) for l in range(L)]
        distinct = sum(int((lay[l][0] > 0).sum()) for l in range(L)) / L
        r = {"T": T, "BM": BM, "distinct_experts": round(distinct, 1),
             "router_linear_ms": graph_ms(lambda l: ops.linear(x[l], router[l]), L, a.reps),
             "route_ms": graph_ms(lambda l: ops.moe_route(logits[l], k, True), L, a.reps),
             "align_ms": graph_ms(lambda l: ops.moe_align(routed[l][0], E, BM), L, a.reps),
             "gemm_swiglu_ms": graph_ms(lambda l: ops.moe_gemm(x[l], gate_up[l], lay[l][2], lay[l][3], k,
                                                               ops.MOE_EPI_SWIGLU, BM), L, a.reps),
             "gemm_down_ms": graph_ms(lambda l: ops.moe_gemm(act[l], down[l], lay[l][2], lay[l][3], k,
                                                             ops.MOE_EPI_PLAIN, BM), L, a.reps),
             "combine_ms": graph_ms(lambda l: ops.moe_combine(y[l], lay[l][4], routed[l][1]), L, a.reps),
             "moe_mlp_ms": graph_ms(lambda l: ops.moe_mlp(x[l], router[l], gate_up[l], down[l], k, True), L, a.reps)}
        if gate_up_q is not None:
            act_q = [ops.moe_gemm(x[l], gate_up_q[l], lay[l][2], lay[l][3], k, ops.MOE_EPI_SWIGLU, BM) for l in range(L)]
            r["fp8_gemm_swiglu_ms"] = graph_ms(lambda l: ops.moe_gemm(x[l], gate_up_q[l], lay[l][2], lay[l][3], k,
                                                                      ops.MOE_EPI_SWIGLU, BM), L, a.reps)
            r["fp8_gemm_down_ms"] = graph_ms(lambda l: ops.moe_gemm(act_q[l], down_q[l], lay[l][2], lay[l][3], k,
                                                                    ops.MOE_EPI_PLAIN, BM), L, a.reps)
            r["fp8_moe_mlp_ms"] = graph_ms(lambda l: ops.moe_mlp(x[l], router[l], gate_up_q[l], down_q[l], k, True),
                                           L, a.reps)
            r["fp8_expert_GBps"] = distinct * expert_bytes_q / (
                (r["fp8_gemm_swiglu_ms"] + r["fp8_gemm_down_ms"]) * 1e-3) / 1e9
        # the per-expert torch loop: host read-back per layer, so a host clock around a synchronise
        for _ in range(2):
            ops.moe_mlp_ref(x[0], router[0], gate_up[0], down[0], k, True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 0
        while n < 2 * L and (n < L or time.perf_counter() - t0 < 1.0):
            ops.moe_mlp_ref(x[n % L], router[n % L], gate_up[n % L], down[n % L], k, True)
            n += 1
        torch.cuda.synchronize()
        r["torch_loop_ms"] = (time.perf_counter() - t0) * 1000 / n
        # bytes the grouped GEMMs must stream, and skinny_gemm on a dense projection of as many bytes
        nbytes = distinct * expert_bytes
        r["expert_GBps"] = nbytes / ((r["gemm_swiglu_ms"] + r["gemm_down_ms"]) * 1e-3) / 1e9
        N = max(16, int(nbytes / (2 * H)) // 16 * 16)
        M = min(T, 32)
        dense = [(rn(N, H) / H ** 0.5).bfloat16() for _ in range(L)]
        outs = [torch.empty(M, N, dtype=torch.bfloat16, device=dev) for _ in range(L)]
        r["skinny_M"] = M
        r["skinny_ms"] = graph_ms(lambda l: torch.ops.dgi.skinny_gemm(outs[l], x[l][:M], dense[l], None, 0), L, a.reps)
        r["skinny_GBps"] = N * H * 2 / (r["skinny_ms"] * 1e-3) / 1e9
        del dense, outs
        rows.append({kk: (round(v, 4) if isinstance(v, float) else v) for kk, v in r.items()})
        print(json.dumps(rows[-1]), flush=True)
    cols = ["T", "BM", "distinct_experts", "moe_mlp_ms", "torch_loop_ms", "router_linear_ms", "route_ms", "align_ms",
            "gemm_swiglu_ms", "gemm_down_ms", "combine_ms", "expert_GBps", "skinny_GBps"]
    if gate_up_q is not None:
        cols += ["fp8_moe_mlp_ms", "fp8_gemm_swiglu_ms", "fp8_gemm_down_ms", "fp8_expert_GBps"]
    print("| " + " | ".join(cols) + " |")
    print("|" + "---|" * len(cols))
    for r in rows:
        print("| " + " | ".join(str(r[c]) for c in cols) + " |")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"hidden": H, "inter": I, "experts": E, "topk": k, "layers": L,
                       "expert_quant": a.expert_quant, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
