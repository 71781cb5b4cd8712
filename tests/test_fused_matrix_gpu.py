"""GPU: the fused pass kernels (csrc/hip/fused.hip k_fused_tile / k_fused_staged, the generated
kernels of jit.hip) on every operand class, from dense random states.

tests/test_pergate_matrix_gpu.py pins the per-gate kernels one gate at a time; this is its
counterpart for the passes, which branch on far more.  Every case of tests/fused_cases.py runs
through StateVector.fromHost -> run(c, RunMode.Fused) -> toHost against the dense numpy reference
(checked against the host mirror of the kernels on the CPU, tests/test_fused_matrix_cpu.py):
amplitudes outside the circuit's subspace bit-identical, circuits of exact ops at tolerance 0, the
rest at 1e-12 per component; the classes hit must cover fused_cases.required in full.

  * test_matrix_interpreter: the pass interpreter at the natural sizes (n = 6..9 k_fused_tile<0..3>,
    10 and 11 staged h = 4 and 5, 12 one 12-qubit tile, 13 and 14 with tile-id bits), at forced
    heights on larger states (h = 0..5 at n = h + 8; h = 7 at n = 14 and 15 with both stage widths,
    and the demotion of a 13-qubit plan's pass to a 12-qubit tile), and without tile-constant
    controls.
  * test_generated_kernels: every staged configuration through the generated kernels, with few
    circuits per size (one hipRTC compile each): the cases pooled, plus the steered cases that the
    pooled circuits do not cover (fused_cases.generated_circuits).  Every staged pass must have run
    as a generated kernel and the classes they took must cover fused_cases.required in full.
  * test_more_than_512_h_in_one_pass: the kMaxUnnormH cap in the interpreter.  A generated pass
    holds at most 192 ops (jit.hip kJitMaxOps), so the cap cannot be reached there.
  * test_relayout_passes_from_a_dense_state: a circuit wider than one tile run six times in a
    row from fromHost.  The first run of a dense state never takes a relayout plan (run.hip
    qsim_run chooses one for a basis state only), but the second identical run arms the
    run-sharing cycle, whose joint plan is a relayout plan; interpreter and generated kernels.
  * test_every_compiled_variant: the knobs read once per process, in child processes
    (tests/fused_child.py).

Not covered here, each with oracle tests of its own: the Pauli-frame arms (FR = true, batched noisy
runs), sub-space launches (fix_mask, the sharded engine), the density-matrix passes.
"""
import json
import os
import subprocess
import sys
import time

import pytest

import fused_cases as fc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture
def plan(qsim):
    from qsim_amd import plan
    yield plan
    fc.restore_settings(plan)


@pytest.mark.parametrize("s", fc.IN_PROCESS, ids=lambda s: s["name"])
def test_matrix_interpreter(qsim, gpu_ready, plan, s):
    plan.set_jit(0, -1)
    fc.apply_settings(plan, s)
    t0 = time.perf_counter()
    ran, worst, failures, hit = fc.run_matrix(qsim, s)
    print(f"{s['name']}: {ran} cases, worst component error {worst:.3e}, {time.perf_counter() - t0:.2f} s")
    assert not failures, "\n".join(failures)
    assert ran == len(fc.cases(s))
    missing = fc.missing(fc.required(s), hit)
    assert not missing, missing


@pytest.mark.parametrize("s", fc.GENERATED, ids=lambda s: s["name"])
def test_generated_kernels(qsim, gpu_ready, plan, s):
    plan.set_jit(2, 0)
    fc.apply_settings(plan, s)
    t0 = time.perf_counter()
    ran, worst, failures, hit, jit_passes, multi = fc.run_generated(qsim, s)
    print(f"{s['name']}: {ran} circuits, {jit_passes} generated passes ({multi} of several stages), worst "
          f"component error {worst:.3e}, {time.perf_counter() - t0:.2f} s")
    assert not failures, "\n".join(failures)
    assert ran >= 1 and jit_passes >= ran and multi >= 1
    missing = fc.missing(fc.required(s), hit)
    assert not missing, missing


def test_more_than_512_h_in_one_pass(qsim, gpu_ready, plan):
    """600 H on 12 qubits in one pass: 512 run as the unnormalised butterfly (the store scales by
    2^-256), the other 88 as the normalised general matrix."""
    plan.set_jit(0, -1)
    n, gates = 12, fc.many_h_circuit()
    c = fc.circuit_of(qsim, n, gates)
    info = plan.plan_stage_info(c)
    assert len(info["passes"]) == 1 and info["passes"][0]["hu_count"] == 512
    psi = fc.dense_state(n, 4242)
    want, may = fc.reference(n, psi, gates)
    sv = qsim.StateVector(n)
    try:
        sv.fromHost(psi)
        sv.run(c, qsim.RunMode.Fused)
        assert sv.lastRunInfo() == (1, 0)
        err = fc.check(sv.toHost(), psi, want, may, info)
    finally:
        sv.close()
    print(f"1 case, worst component error {err:.3e}")


@pytest.mark.parametrize("jit", [0, 2])
@pytest.mark.parametrize("seed", [0, 1])
def test_relayout_passes_from_a_dense_state(qsim, gpu_ready, plan, jit, seed):
    """16 qubits is the smallest size with relayout plans (relayout.hip: a 12-qubit tile and a
    4-qubit run).  Runs 1 and 2 execute the fixed-layout plan; run 2 arms the cycle of 4 copies,
    runs 3 to 6 are its calls and complete it, so toHost reads six copies of the circuit."""
    n, runs = 16, 6
    plan.set_relabel(1, n)
    plan.set_relayout(1, n)
    plan.set_calibrate(0, -1)
    plan.set_run_share(1, 4)
    plan.set_jit(jit, 0 if jit else -1)
    gates = fc.relayout_circuit(n, seed)
    c = fc.circuit_of(qsim, n, gates)
    joint, single, _ = plan.plan_share_info(c, 4)
    assert 0 < joint < 4 * single
    psi = fc.dense_state(n, 77 + seed)
    want = psi
    for _ in range(runs):
        want, _ = fc.reference(n, want, gates)
    sv = qsim.StateVector(n)
    try:
        sv.fromHost(psi)
        launched = []
        for _ in range(runs):
            sv.run(c, qsim.RunMode.Fused)
            launched.append(sv.lastRunInfo())
        assert sv.layoutInfo()["relayout"], "the run-sharing cycle was not armed"
        # the four calls of the cycle launch the joint plan's passes, all of them generated with jit
        assert sum(p for p, _ in launched[2:]) == joint, (launched, joint)
        assert all(j == (p if jit else 0) for p, j in launched[2:]), launched
        got = sv.toHost()
    finally:
        sv.close()
    err = float(max(abs(got.real - want.real).max(), abs(got.imag - want.imag).max()))
    print(f"jit={jit} seed={seed}: 1 case of {runs} runs, worst component error {err:.3e}")
    assert err <= fc.TOL


# Measured on an MI355X, start-up and first kernel load included: the default-width child (rb4,
# n = 13 and 14, 867 cases) takes 1.04 to 1.15 s wall and is the slowest of the six interpreter
# children (0.46 to 1.15 s); the two generated-kernel children (24 circuits, one hipRTC compile
# each) take 4.66 s and 6.23 s; all eight together 14.8 s.  Times five for process start-up on a
# busy machine.  In process the slowest test_generated_kernels case (16 compiles) takes 4.3 s.
CHILD_SECONDS = {False: 1.2, True: 6.3}  # by "runs the generated kernels"


@pytest.mark.subprocess  # children start before this process initialises the GPU, one at a time
def test_every_compiled_variant():
    base = {k: v for k, v in os.environ.items() if k not in fc.KNOBS}
    ran = 0
    for idx, variant in enumerate(fc.CHILDREN):  # the first failing child ends the test
        env = dict(base, **{k: str(v) for k, v in variant[0]["env"].items()})
        t0 = time.perf_counter()
        r = subprocess.run([sys.executable, os.path.join(HERE, "fused_child.py"), str(idx)],
                           capture_output=True, text=True,
                           timeout=5 * CHILD_SECONDS[bool(variant[0].get("jit"))], env=env)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert lines, (variant[0]["name"], r.returncode, r.stderr[-3000:])
        out = json.loads(lines[-1])
        print(variant[0]["name"], out["cases"], out["worst"], f"{time.perf_counter() - t0:.2f} s")
        assert r.returncode == 0 and out["failures"] == [] and out["missing"] == [], (
            variant[0]["name"], r.returncode, out["failures"], out["missing"], r.stderr[-3000:])
        if variant[0].get("jit"):
            # (the circuits are chosen from the plans, which depend on the child's knobs: the child
            # counts them; every one ran as generated kernels, some passes with several stages,
            # which is what QSIM_JIT_PIPE acts on)
            assert out["cases"] >= 2 and out["jit_passes"] >= out["cases"] and out["multi_stage"] >= 1, out
        else:
            want = sum(len(fc.cases(s)) for s in variant)
            assert out["cases"] == want, (variant[0]["name"], out["cases"], want)
        assert out["worst"] <= fc.TOL
        ran += 1
    assert ran == 8
