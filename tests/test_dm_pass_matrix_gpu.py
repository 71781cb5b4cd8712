"""GPU: the density-matrix passes on every operand class, from dense general matrices.

Every case of tests/dm_pass_cases.py runs through state.fromHost -> DensityMatrixSimulator.run ->
getDensityMatrix against the Kraus / unitary numpy reference (checked against the oracle and
against the host mirror of the kernels on the CPU, tests/test_dm_pass_matrix_cpu.py): elements
outside the circuit's may-change mask bit-identical, circuits of exact ops at tolerance 0, the rest
at 1e-12 per component; the classes hit must cover dm_pass_cases.required in full.

  * test_matrix_interpreter: the pass interpreter (k_fused_tile, k_fused_staged) and the same case
    list in RunMode.PerGate, at the natural sizes n = 3..8, at forced tile heights 0..5, at height 7
    with both stage widths (and its demotion to 12-bit tiles), without tile-constant controls.
  * test_generated_kernels: a greedy cover of the required classes through the generated kernels;
    every pass must have run as one.
  * test_apply_channel: applyChannel of every type on every qubit at n = 3, 6, 7.
  * test_every_compiled_variant: the knobs read once per process and the relabeled configurations
    (the case runs second, under the labels of a first run), in child processes
    (tests/dm_pass_child.py).
"""
import json
import os
import subprocess
import sys
import time

import pytest

import dm_pass_cases as dc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture
def plan(qsim):
    from qsim_amd import plan
    yield plan
    dc.restore_settings(plan)
    plan.set_jit(1, 20)


@pytest.mark.parametrize("s", dc.IN_PROCESS, ids=lambda s: s["name"])
def test_matrix_interpreter(qsim, gpu_ready, plan, s):
    plan.set_jit(0, -1)
    dc.apply_settings(plan, s)
    t0 = time.perf_counter()
    ran, worst, failures, hit = dc.run_matrix(qsim, s)
    print(f"{s['name']}: {ran} cases fused and per-gate, worst component error {worst:.3e}, "
          f"{time.perf_counter() - t0:.2f} s")
    assert not failures, "\n".join(failures)
    assert ran == len(dc.cases(s))
    missing = dc.missing(dc.required(s), hit)
    assert not missing, missing


@pytest.mark.parametrize("s", dc.GENERATED, ids=lambda s: s["name"])
def test_generated_kernels(qsim, gpu_ready, plan, s):
    plan.set_jit(2, 0)
    dc.apply_settings(plan, s)
    t0 = time.perf_counter()
    try:
        ran, worst, failures, hit = dc.run_generated(qsim, s)
    finally:
        plan.set_jit(1, 20)
    print(f"{s['name']}: {ran} circuits, worst component error {worst:.3e}, {time.perf_counter() - t0:.2f} s")
    assert not failures, "\n".join(failures)
    assert 1 <= ran <= dc.MAX_GENERATED
    missing = dc.missing(dc.required(s), hit)
    assert not missing, missing


@pytest.mark.parametrize("n", [3, 6, 7])
def test_apply_channel(qsim, gpu_ready, n):
    ran, worst, failures = dc.run_channels(qsim, n)
    print(f"n={n}: {ran} channels, worst component error {worst:.3e}")
    assert not failures, "\n".join(failures)
    assert ran == 6 * n


@pytest.mark.subprocess  # children start before this process initialises the GPU, one at a time
def test_every_compiled_variant():
    base = {k: v for k, v in os.environ.items() if k not in dc.KNOBS}
    ran = 0
    for idx, variant in enumerate(dc.CHILDREN):  # the first failing child ends the test
        env = dict(base, **{k: str(v) for k, v in variant[0]["env"].items()})
        t0 = time.perf_counter()
        r = subprocess.run([sys.executable, os.path.join(HERE, "dm_pass_child.py"), str(idx)],
                           capture_output=True, text=True, timeout=120, env=env)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert lines, (variant[0]["name"], r.returncode, r.stderr[-3000:])
        out = json.loads(lines[-1])
        print(variant[0]["name"], out["per_config"], f"{time.perf_counter() - t0:.2f} s")
        assert r.returncode == 0 and out["failures"] == [] and out["missing"] == [], (
            variant[0]["name"], r.returncode, out["failures"], out["missing"], r.stderr[-3000:])
        assert out["cases"] >= len(variant) and out["worst"] <= dc.TOL
        ran += 1
    assert ran == len(dc.CHILDREN)
