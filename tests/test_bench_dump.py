"""bench.py --dump-outputs: what the timed path computed, written as .npy files that two builds can be compared by.
The CPU test checks the sampling and the files; the GPU test runs the bench twice and requires the same outputs bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_field_sample_is_fixed_and_within_budget(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    psi = torch.from_numpy(np.random.default_rng(1).standard_normal(3 * bench.DUMP_SAMPLE // 2))
    a, b = bench.field_sample("psi", psi), bench.field_sample("psi", psi.clone())
    assert sorted(a) == ["psi", "psi_cells"]
    cells = a["psi_cells"].astype(np.int64)
    assert cells.shape == (bench.DUMP_SAMPLE,) and np.all(np.diff(cells) > 0) and np.array_equal(a["psi_cells"], b["psi_cells"])
    assert np.array_equal(a["psi"], psi.numpy()[cells])
    small = bench.field_sample("x", psi[:1000])
    assert list(small) == ["x"] and np.array_equal(small["x"], psi.numpy()[:1000])
    bench.dump_outputs(str(tmp_path), {**a, "history": np.arange(5.0)})
    files = sorted(os.listdir(tmp_path))
    assert files == ["history.npy", "psi.npy", "psi_cells.npy"]
    assert all(np.load(tmp_path / f).dtype == np.float64 for f in files)
    assert sum(os.path.getsize(tmp_path / f) for f in files) <= 64 << 20


def test_full_is_an_option_and_off_by_default():
    """a plain `--gpus 1 --steps N --warmup W` run asks for none of the extra measurements; --full asks for them, and the options
    that take single legs out of a --full run are still understood"""
    sys.path.insert(0, ROOT)
    import bench
    plain = bench.make_parser().parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert plain.full is False and (plain.gpus, plain.steps, plain.warmup, plain.repeats, plain.dump_outputs) == (1, 20, 5, 5, None)
    full = bench.make_parser().parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5", "--full", "--no-cpu", "--no-supplements"])
    assert full.full is True and full.no_cpu and full.no_supplements and (full.steps, full.warmup, full.repeats) == (20, 5, 5)


@pytest.mark.gpu
def test_dump_outputs_repeat_bit_for_bit(tmp_path):
    steps, warmup, repeats = 7, 2, 3
    dumps = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--warmup", str(warmup), "--repeats", str(repeats),
                              "--dims", "40", "32", "24", "--no-cpu", "--no-supplements", "--dump-outputs", str(d)],
                             capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        dumps.append({f[:-4]: np.load(d / f) for f in os.listdir(d)})
    a, b = dumps
    assert sorted(a) == ["history", "psi"] and a["psi"].shape == (40 * 32 * 24,)
    assert a["history"].shape == (warmup + repeats * steps + 1,) and np.all(np.isfinite(a["psi"]))
    assert a["history"][-1] < a["history"][0]
    for name in a:
        assert np.array_equal(a[name], b[name]), name
