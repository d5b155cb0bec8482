"""Driver-contract regression tests for bench.py: single-process CPU run
and a 2-process gloo torchrun launch must both print the JSON line."""

import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_json(line: str, n_gpus: int):
    row = json.loads(line)
    assert row["metric"] == "train_graphs_per_sec"
    assert row["n_gpus"] == n_gpus
    assert row["value"] > 0 and row["ms_per_step"] > 0
    assert row["scaling"] == "weak"
    assert row["config"]["global_batch"] == 8 * n_gpus
    return row


def test_bench_single_process_cpu():
    out = subprocess.run(
        [sys.executable, "bench.py", "--steps", "2", "--warmup", "1",
         "--model", "ddfa", "--batch", "8", "--n-batches", "2"],
        cwd=REPO, capture_output=True, text=True, timeout=300,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    _check_json(out.stdout.strip().splitlines()[-1], 1)


def test_bench_dump_outputs_repeatable(tmp_path):
    """--dump-outputs writes the dump step's arrays as float32 .npy. The dump
    step is the timed path run on the last timed step's batch from the seeded
    start state, so it does not depend on how many steps trained before it:
    3 timed + 1 warmup steps and 1 timed step (both end on batch 0 of 2) must
    dump the same arrays (the CPU path has no atomics: bit for bit). --full
    is accepted and leaves the result line unchanged in meaning."""
    import numpy as np

    dumps = []
    for name, steps, warmup, extra in (("a", 3, 1, []), ("b", 1, 0, ["--full"])):
        d = tmp_path / name
        out = subprocess.run(
            [sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps),
             "--warmup", str(warmup), "--batch", "8", "--n-batches", "2",
             "--dump-outputs", str(d)] + extra,
            cwd=REPO, capture_output=True, text=True, timeout=300,
        )
        assert out.returncode == 0, out.stderr[-2000:]
        row = _check_json(out.stdout.strip().splitlines()[-1], 1)
        assert row["steps"] == steps and row["warmup"] == warmup
        files = sorted(p.name for p in d.iterdir())
        assert files == ["grads.npy", "loss.npy", "params.npy"]
        arrs = {f: np.load(d / f) for f in files}
        for f, a in arrs.items():
            assert a.dtype == np.float32 and a.size > 0 and np.isfinite(a).all(), f
        assert sum(a.nbytes for a in arrs.values()) <= 64 * 1024 * 1024
        assert arrs["loss.npy"].shape == (1,)
        assert arrs["params.npy"].shape == arrs["grads.npy"].shape
        assert np.abs(arrs["grads.npy"]).max() > 0
        dumps.append(arrs)
    for f in dumps[0]:
        np.testing.assert_array_equal(dumps[0][f], dumps[1][f])


def test_bench_torchrun_two_ranks_gloo():
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29619", "bench.py", "--gpus", "2", "--steps", "2",
         "--warmup", "1", "--model", "ddfa", "--batch", "8", "--n-batches", "2"],
        cwd=REPO, capture_output=True, text=True, timeout=600,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    json_lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(json_lines) == 1  # rank 0 only
    _check_json(json_lines[-1], 2)
