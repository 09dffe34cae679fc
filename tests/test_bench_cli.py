"""bench.py's command line and its --dump-outputs writer, without a GPU (the timed runs themselves are in test_gpu_pipeline.py)."""
import os
import subprocess
import sys

import numpy as np

from conftest import ROOT

import bench


def run_cli(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), capture_output=True, text=True, timeout=300, cwd=ROOT)


def test_help_lists_full_and_dump_outputs():
    r = run_cli("--help")
    assert r.returncode == 0, r.stderr
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


def test_steps_must_be_at_least_one():
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        r = run_cli(*bad)
        assert r.returncode == 2 and "--steps must be >= 1" in r.stderr, (bad, r.stderr)


def test_dump_outputs_whole_when_it_fits(tmp_path):
    import torch
    x = torch.arange(6 * 5 * 3, dtype=torch.uint8).reshape(6, 5, 3)
    bench.dump_outputs(str(tmp_path), "output", x, 1 << 20)
    got = np.load(str(tmp_path / "output.npy"))
    assert got.dtype == np.float32 and np.array_equal(got, x.numpy().astype(np.float32))


def test_dump_outputs_samples_fixed_rows_within_the_budget(tmp_path):
    import torch
    x = torch.from_numpy(np.random.default_rng(3).random((1000, 64), dtype=np.float32))
    budget = 100 * 64 * 4 + 17
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), "output", x, budget)
    a, b = (np.load(str(tmp_path / d / "output.npy")) for d in ("a", "b"))
    assert a.shape == (100, 64) and a.dtype == np.float32 and np.array_equal(a, b)     # the same rows every run
    assert os.path.getsize(str(tmp_path / "a" / "output.npy")) <= budget + 128          # (+ the .npy header)
    rows = [int(np.flatnonzero((x.numpy() == r).all(axis=1))[0]) for r in a]
    assert rows == sorted(set(rows))                                                     # whole rows, in order
