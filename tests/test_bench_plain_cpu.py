"""A plain ``bench.py --gpus 1 --steps N --warmup W`` run on CPU (llama-tiny): the seeded
steady-state population against the step-by-step ramp of ``--full``, ``--steps`` as the number
of timed steps, and ``--dump-outputs`` (float arrays, the same from run to run)."""
import glob
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = ["--model", "llama-tiny", "--concurrency", "8", "--output-len", "8", "--prompt-len", "32",
        "--max-batched-tokens", "256", "--no-graphs"]


def _run_single(monkeypatch, *extra):
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench.torch.cuda, "is_available", lambda: False)     # the CPU engine, wherever this runs
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", *TINY, *extra])
    return bench, bench.run_single(bench.parse())


def test_seeded_population_is_the_one_the_ramp_ends_with():
    """conc 8, 8 output tokens: one sequence of every age 1..7, context prompt + age - 1, as many
    tokens to go as a request admitted that many steps ago, its KV pages allocated."""
    sys.path.insert(0, ROOT)
    import random
    import bench
    from dgi.engine import EngineConfig, LLMEngine
    from dgi.sched.request import SamplingParams, Status
    eng = LLMEngine(EngineConfig(model="llama-tiny", device="cpu", max_num_seqs=8, max_num_batched_tokens=256,
                                 max_model_len=2048, use_graphs=False, enable_prefix_caching=False))
    rng = random.Random(0)
    vocab = eng.model_cfg.vocab_size
    sp = SamplingParams(max_tokens=8, temperature=0.0, ignore_eos=True)
    reqs = bench.seed_steady_state(eng, lambda: bench._prompt(rng, 32, vocab), sp, 8, seed=0)
    assert [len(r.output) for r in reqs] == [1] * 7
    assert [len(r.prompt) for r in reqs] == [32 + g - 1 for g in range(7, 0, -1)]          # oldest first
    assert [r.params.max_tokens - len(r.output) for r in reqs] == [8 - g for g in range(7, 0, -1)]
    assert all(r.status is Status.RUNNING and r.num_computed == r.total_len - 1 for r in reqs)
    bs = eng.pool.block_size
    assert all(len(r.blocks) == -(-len(r.prompt) // bs) for r in reqs)
    assert sp.max_tokens == 8                                                                # the caller's params are untouched
    # the oldest ends at the next step, and the engine then holds the 6 others
    outs = eng.step()
    assert len(outs) == 7 and [o.finished for o in outs] == [True] + [False] * 6


def test_plain_run_times_the_steps_the_full_ramp_reaches(monkeypatch):
    """The seeded population and --full's step-by-step ramp reach the same steady state: the timed
    steps sample the same number of tokens and leave the same sequences running; --steps is the
    number of timed steps in both."""
    bench, plain = _run_single(monkeypatch, "--steps", "5", "--warmup", "2")
    _, full = _run_single(monkeypatch, "--steps", "5", "--warmup", "2", "--full")
    assert plain["ramp"] == {"kind": "seeded", "steps": bench.SETTLE_STEPS, "seeded_requests": 7}
    assert full["ramp"] == {"kind": "steps", "steps": 8, "seeded_requests": 0}
    assert plain["engine"]["steps"] == bench.SETTLE_STEPS + 2 + 5
    assert full["engine"]["steps"] == 8 + 2 + 5
    assert plain["phases"]["execute"]["n"] == full["phases"]["execute"]["n"] == 5      # the timed steps
    assert plain["tokens"] == full["tokens"] == 5 * 8
    assert plain["stats"]["running"] == full["stats"]["running"] == 7
    assert len(plain["ttfts"]) == len(full["ttfts"]) == 5                                # one new prompt a step
    # an explicit --ramp-steps keeps the step-by-step ramp
    _, ramped = _run_single(monkeypatch, "--steps", "2", "--warmup", "1", "--ramp-steps", "3")
    assert ramped["ramp"]["kind"] == "steps" and ramped["engine"]["steps"] == 3 + 1 + 2


def test_dump_outputs_same_arguments_same_arrays(tmp_path):
    """Two runs with the same arguments write the same float arrays: the last timed step's tokens
    and the logits rows they are the argmax of."""
    lines = []
    for name in ("a", "b"):
        cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", *TINY,
               "--dump-outputs", str(tmp_path / name)]
        r = subprocess.run(cmd, cwd=ROOT, env={**os.environ, "OMP_NUM_THREADS": "1", "HIP_VISIBLE_DEVICES": "",
                                                   "CUDA_VISIBLE_DEVICES": ""},          # the CPU engine, wherever this runs
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-3000:]
        lines.append(json.loads([x for x in r.stdout.splitlines() if x.startswith('{"metric"')][-1]))
    d = lines[0]
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "tokens/s" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0 and d["value"] > 0 and d["dtype"] == "bf16"
    assert d["extra"]["ramp"]["kind"] == "seeded"
    names = sorted(os.path.basename(p) for p in glob.glob(str(tmp_path / "a" / "*.npy")))
    assert names == ["logits.npy", "logits_columns.npy", "output_index.npy", "request_ids.npy", "tokens.npy"]
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all()
        assert a.shape == b.shape and np.array_equal(a, b), n
        assert d["extra"]["dumped"][n[:-4]] == list(a.shape)
        total += a.nbytes
    assert total <= 64 << 20
    tokens, logits = np.load(tmp_path / "a" / "tokens.npy"), np.load(tmp_path / "a" / "logits.npy")
    cols = np.load(tmp_path / "a" / "logits_columns.npy")
    assert tokens.shape == (8,) and logits.shape == (8, len(cols))       # 7 decode rows + 1 new prompt
    assert np.array_equal(cols[logits.argmax(1)], tokens)                # greedy: every column fits the allowance


def test_dump_sample_stays_inside_the_allowance(tmp_path):
    """A logits block larger than the allowance is written as a fixed, seeded sample of its columns."""
    sys.path.insert(0, ROOT)
    import types
    import torch
    import bench
    outs = [types.SimpleNamespace(token=i, rid=i, request=types.SimpleNamespace(output=[0, i])) for i in range(4)]
    logits = torch.arange(4 * 1000, dtype=torch.float32).view(4, 1000)
    old = bench.DUMP_LOGIT_BYTES
    bench.DUMP_LOGIT_BYTES = 4 * 4 * 100                                  # room for 100 columns of 4 rows
    try:
        s1 = bench.dump_outputs(str(tmp_path / "x"), outs, logits, seed=0)
        s2 = bench.dump_outputs(str(tmp_path / "y"), outs, logits, seed=0)
    finally:
        bench.DUMP_LOGIT_BYTES = old
    assert s1 == s2 and s1["logits"] == [4, 100]
    cols = np.load(tmp_path / "x" / "logits_columns.npy")
    assert np.array_equal(cols, np.load(tmp_path / "y" / "logits_columns.npy"))
    assert len(set(cols)) == 100 and (np.diff(cols) > 0).all()
    assert np.array_equal(np.load(tmp_path / "x" / "logits.npy"), logits.numpy()[:, cols.astype(int)])
    assert np.load(tmp_path / "x" / "output_index.npy").tolist() == [1.0] * 4
