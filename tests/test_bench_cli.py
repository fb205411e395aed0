"""bench.py's command line, rehearsed on CPU (MMDYN_BENCH_DRYRUN=emu: emulated kernels, one rank): a plain run prints the
headline line and nothing of --full, --full adds the roofline object, and --dump-outputs writes what the last timed step
computed -- float32 / float64 arrays within 64 MB, identical from run to run of the same arguments."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(MMDYN_BENCH_DRYRUN="emu")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", "2"] + list(args)
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_plain_run_is_lean_and_full_adds_the_roofline():
    d = _bench("--steps", "3", "--warmup", "1")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 3 and d["warmup"] == 1
    assert d["value"] == pytest.approx(2 * 3 / (d["ms_per_step"] * 3e-3), rel=1e-6)
    assert not {"roofline", "native_fp32", "alt_arithmetic", "cpu_baseline"} & set(d)
    f = _bench("--steps", "1", "--warmup", "0", "--full")
    assert "roofline" in f and f["steps"] == 1


def test_dump_outputs_same_arrays_every_run(tmp_path):
    dirs = [tmp_path / "a", tmp_path / "b"]
    for d in dirs:
        _bench("--steps", "2", "--warmup", "1", "--dump-outputs", str(d))
    names = sorted(os.path.basename(f) for f in glob.glob(str(dirs[0] / "*.npy")))
    assert names == ["buffers.npy", "loss.npy", "params.npy", "partials.npy"]
    assert sum(os.path.getsize(f) for f in glob.glob(str(dirs[0] / "*.npy"))) <= 64 * 10 ** 6
    for n in names:
        a, b = np.load(dirs[0] / n), np.load(dirs[1] / n)
        assert a.dtype in (np.float32, np.float64) and a.size > 0, n
        assert np.isfinite(a).all(), n
        np.testing.assert_array_equal(a, b, err_msg=n)
    assert np.load(dirs[0] / "partials.npy").shape == (7,)


def test_dump_outputs_samples_beyond_the_budget(tmp_path, monkeypatch):
    """Arrays above the budget are replaced by the same seeded sample every time; small ones stay whole."""
    import torch
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 3 * 2 ** 20)
    big = torch.arange(2 ** 21, dtype=torch.float32)           # 8 MB
    small = torch.arange(10, dtype=torch.float64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), [("big", big), ("small", small)])
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    np.testing.assert_array_equal(a, b)
    assert a.dtype == np.float32 and 0 < a.nbytes <= 3 * 2 ** 20 and np.all(np.diff(a) > 0)
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float64 and s.tolist() == list(range(10))
