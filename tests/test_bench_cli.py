"""bench.py's command line: a plain run measures the headline only, --full everything else, and
--dump-outputs writes what the last timed step left.

CPU: the option gating (no engine needed).  GPU: `bench.py --dump-outputs` in a child process at
20 qubits (the state written whole) and 21 qubits (the seeded sample of 1024 x 1024 amplitudes),
each compared with the same number of runs of the same circuit in this process.
"""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_cli", BENCH)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", [BENCH, *argv])
    return _bench_module().parse()


def test_plain_run_measures_the_headline_only(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    assert a.no_extras and a.no_1q28 and a.no_batch16 and a.cpu_budget == 0


def test_full_run_keeps_every_object(monkeypatch):
    a = _parse(monkeypatch, "--full")
    assert a.full and not (a.no_extras or a.no_1q28 or a.no_batch16) and a.cpu_budget == 12.0
    assert set(a.extras.split(",")) >= {"seeds", "default_mode", "w_ref", "w_hc_28q", "dm", "noisy"}
    a = _parse(monkeypatch, "--full", "--cpu-budget", "1", "--no-extras")
    assert a.no_extras and not a.no_1q28 and a.cpu_budget == 1.0


def test_dump_outputs_needs_a_one_gpu_run(tmp_path):
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dry-run", "--dump-outputs", str(tmp_path / "d")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--dump-outputs" in r.stderr
    assert not (tmp_path / "d").exists()


@pytest.mark.gpu
@pytest.mark.subprocess
@pytest.mark.parametrize("n", [20, 21])
def test_dump_outputs_holds_the_last_steps_state(qsim, tmp_path, n):
    steps, warmup, seed = 2, 1, 7
    d = tmp_path / "out"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--qubits", str(n), "--seed", str(seed), "--dump-outputs", str(d)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["steps"] == steps and out["ms_per_step"] > 0 and out["cpu_baseline"] is None
    assert not {"roofline_1q28", "roofline_batch16", "seeds", "w_ref", "dm_14q", "noisy_26q"} & set(out)
    got = np.load(d / "state_vector.npy")
    assert got.dtype == np.float64 and got.shape == (1 << 20, 2)  # 16 MiB at both sizes
    # the same runs here: bench.py warms up `warmup` times, then times `steps` runs, no reset between
    c = qsim.createRandomHCCircuit(n, 100, seed)
    sim = qsim.Simulator(n)
    for _ in range(warmup + steps):
        sim.run(c)
    ref = sim.getStateVector()
    del sim
    if n == 20:
        assert sorted(p.name for p in d.iterdir()) == ["state_vector.npy"]
    else:
        idx = np.load(d / "state_vector_index.npy")
        assert idx.dtype == np.float64 and idx.shape == (1 << 20,)
        idx = idx.astype(np.int64)
        runs = idx.reshape(1024, 1024)
        assert np.all(np.diff(runs, axis=1) == 1) and np.all(runs[:, 0] % 1024 == 0)
        assert len(set(runs[:, 0])) == 1024 and 0 <= idx.min() and idx.max() < 1 << n
        rng = np.random.default_rng(seed)  # the documented draw
        assert np.array_equal(runs[:, 0], np.sort(rng.choice((1 << n) // 1024, 1024, replace=False)) * 1024)
        ref = ref[idx]
    err = float(np.max(np.abs(got[:, 0] + 1j * got[:, 1] - ref)))
    assert err < 1e-12, err  # the suite's per-amplitude bar (same engine, possibly another layout)
