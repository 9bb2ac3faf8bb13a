"""bench.py --dump-outputs: what the last timed step computed, written as .npy files that two builds can compare output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_sample_is_fixed_and_the_step_fits_64_mb(tmp_path, monkeypatch):
    """Arrays above the cap are written as the same seeded sample every time; the four arrays of a step stay under 64 MB."""
    import bench
    assert 4 * bench.DUMP_MAX_ELEMS * 4 <= 64 << 20
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 1000)
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3), torch.nn.BatchNorm2d(8), torch.nn.Linear(10, 200))
    out = m(torch.randn(2, 3, 12, 12))
    loss = out.square().mean()
    loss.backward()
    infos = []
    for d in ("a", "b"):
        infos.append(bench.dump_outputs(str(tmp_path / d), bench.step_outputs(m, loss=loss, logits=out.bfloat16())))
    assert infos[0] == infos[1] and set(infos[0]) == {"loss", "logits", "state", "grads"}
    assert infos[0]["logits"] == {"shape": [2, 8, 10, 200], "dtype": "bfloat16", "sampled": 1000}
    assert infos[0]["loss"]["sampled"] is None
    for name in infos[0]:
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, b), name
    assert float(np.load(tmp_path / "a" / "loss.npy")) == float(loss.detach())
    full = out.detach().bfloat16().float().reshape(-1).numpy()
    assert np.isin(np.load(tmp_path / "a" / "logits.npy"), full).all()


@pytest.mark.gpu
def test_bench_dump_outputs_are_the_last_timed_step_and_repeat(tmp_path):
    """Two bench.py runs with the same arguments: --steps timed steps, ms_per_step on the line, and the same loss, logits, model
    state and gradients in the dump, bit for bit; the dumped loss is the line's."""
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    lines, dirs = [], []
    for run in ("a", "b"):
        d = str(tmp_path / run)
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "3", "--batch", "2", "--size", "256",
                              "--no-cpu-baseline", "--no-secondary", "--no-profile", "--no-calibration", "--dump-outputs", d],
                             env=env, capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-2000:]
        lines.append(json.loads([ln for ln in out.stdout.splitlines() if ln.strip()][-1]))
        dirs.append(d)
    for line in lines:
        assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["dumped_outputs"]["dir"] in dirs
        arrays = line["dumped_outputs"]["arrays"]
        assert arrays["logits"]["shape"] == [2, 12, 256, 256] and arrays["loss"]["shape"] == []
    total = 0
    for name in ("loss", "logits", "state", "grads"):
        a, b = (np.load(os.path.join(d, f"{name}.npy")) for d in dirs)
        total += a.nbytes
        assert a.dtype == np.float32 and np.isfinite(a).all() and np.array_equal(a, b), name
    assert total <= 64 << 20
    assert float(np.load(os.path.join(dirs[0], "loss.npy"))) == lines[0]["config"]["loss"]


FULL_ONLY = ("calibration", "value_normalised", "profile_pass", "roofline", "secondary", "cpu_baseline")


@pytest.mark.gpu
def test_plain_run_is_the_headline_of_a_full_run(tmp_path):
    """A plain bench.py run prints the headline alone, and it times and dumps the same steps as a --full run of the same arguments:
    the calibration probes before the timed steps and the bracketed pass behind them change nothing that is dumped."""
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    args = ["--steps", "3", "--warmup", "3", "--batch", "2", "--size", "256"]
    lines, dirs = {}, {}
    for run, extra in (("plain", []), ("full", ["--full", "--no-cpu-baseline", "--no-secondary", "--profile-stride", "2"])):
        dirs[run] = str(tmp_path / run)
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args + extra + ["--dump-outputs", dirs[run]],
                             env=env, capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-2000:]
        stdout = [ln for ln in out.stdout.splitlines() if ln.strip()]
        assert len(stdout) == 1, stdout                # ONE JSON line on stdout
        lines[run] = json.loads(stdout[0])
    plain, full = lines["plain"], lines["full"]
    assert not set(FULL_ONLY) & set(plain), sorted(plain)
    assert {"calibration", "value_normalised", "profile_pass", "roofline"} <= set(full), sorted(full)
    for key in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup"):
        assert plain[key] == full[key], key
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["config"]["launch"] == full["config"]["launch"]
    assert plain["config"]["loss"] == full["config"]["loss"]
    for name in ("loss", "logits", "state", "grads"):
        a, b = (np.load(os.path.join(dirs[run], f"{name}.npy")) for run in ("plain", "full"))
        assert np.array_equal(a, b), name
