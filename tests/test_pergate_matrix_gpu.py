"""GPU: the per-gate kernels (csrc/hip/gates.hip) on every operand class, under every launch variant.

RunMode::PerGate is what the fused, JIT, relayout and sharded tests compare against, so it is
pinned here on its own against the dense numpy reference of tests/pergate_cases.py (checked against
the oracle on the CPU in tests/test_pergate_reference_cpu.py):

  * test_operand_matrix: one gate at a time on a dense random state (fromHost, applyGate, toHost):
    every gate type with targets and controls below and from bit 6, SWAP in ll / lh / hh form,
    one-sided diagonals, and applyMatrix1Q under 1-3 controls.  Amplitudes outside the gate's
    subspace must come back bit-identical; X, Y, Z, S, Sdag, CNOT, CZ, SWAP and Toffoli must equal the
    reference exactly; the rest at 1e-12 per component.
  * test_every_launch_variant: the same matrix in child processes (tests/pergate_child.py) whose
    environment selects each compiled variant: k_m1_slice / _g / _c (QSIM_SLICE_FAR_MODE 0 / 1 / 2),
    k_m1_lane, k_diag at every U in {1, 2, 4, 8}, both QSIM_NT values, the three work-group orders.
  * test_batched_per_gate_equals_oracle: the batch dimension of item_base (trajectory stride)
    against the oracle, at batch sizes that are no power of two and n below 6.
"""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import pergate_cases as pc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


# ---------------------------------------------------------------- default variant, in process
@pytest.mark.parametrize("n", [5, 6, 7, 10, 13])
def test_operand_matrix(qsim, gpu_ready, n):
    """n = 5: 32 live lanes, one wave-item; 7: the slice kernels get one item and three idle waves;
    10, 13: positions 0, 2, 3, 5, 6, 7, n-1 (13: Toffoli only with an operand from bit 6)."""
    ran, worst, failures = pc.run_matrix(qsim, n)
    print(f"n={n}: {ran} cases, worst component error {worst:.3e}")
    assert not failures, "\n".join(failures)
    assert ran == pc.matrix_count(n)


# ---------------------------------------------------------------- every variant, child processes
_FAR = {"QSIM_SLICE_FAR_LO": 6, "QSIM_SLICE_FAR_HI": 63, "QSIM_SLICE_FAR_MIN_QUBITS": 1}
_NEAR = {"QSIM_SLICE_FAR_MIN_QUBITS": 99}
VARIANTS = [
    # every slice target takes the far path: the shipped far kernel (mode 2, 2 items per wave)
    dict(_FAR),
    dict(_FAR, QSIM_SLICE_FAR_MODE=1, QSIM_SLICE_U_FAR=4, QSIM_SLICE_FAR_BMAP=2, QSIM_NT=0),
    dict(_FAR, QSIM_SLICE_FAR_MODE=2, QSIM_SLICE_U_FAR=8, QSIM_SLICE_FAR_BMAP=0),
    dict(_FAR, QSIM_SLICE_FAR_MODE=0, QSIM_SLICE_U_FAR=1),
    # no far path: the other U of k_m1_slice, k_m1_lane and k_diag
    dict(_NEAR, QSIM_SLICE_U=8, QSIM_LANE_U=8, QSIM_DIAG_U=8, QSIM_SLICE_BMAP=2, QSIM_NT=0),
    dict(_NEAR, QSIM_SLICE_U=4, QSIM_LANE_U=1, QSIM_DIAG_U=1, QSIM_SLICE_BMAP=0),
    dict(_NEAR, QSIM_SLICE_U=2, QSIM_LANE_U=4, QSIM_DIAG_U=4, QSIM_SLICE_BMAP=1),
]
KNOBS = ("QSIM_SLICE_U", "QSIM_SLICE_U_FAR", "QSIM_SLICE_FAR_LO", "QSIM_SLICE_FAR_HI",
         "QSIM_SLICE_FAR_MODE", "QSIM_SLICE_FAR_MIN_QUBITS", "QSIM_SLICE_FAR_BMAP", "QSIM_SLICE_BMAP",
         "QSIM_LANE_U", "QSIM_DIAG_U", "QSIM_NT")
# 7: one item, one block (the work-group orders fall back to the natural one); 10: 2-16 items, no
# multiple of 4 U for the larger U, partial last blocks; 16: 128-1024 items, grids divisible by 2
# but not by 8, and by 8
CHILD_SIZES = [7, 10, 16]
# Measured on an MI355X: the default-variant child (these three sizes, 933 cases, start-up and
# first kernel load included) takes 0.61 s wall, the seven children of this test 3.95 s together;
# 0.7 s taken, times five for process start-up on a busy machine.
CHILD_SECONDS = 0.7
CHILD_TIMEOUT = 5 * CHILD_SECONDS


@pytest.mark.subprocess  # children start before this process initialises the GPU, one at a time
def test_every_launch_variant():
    want = sum(pc.matrix_count(n) for n in CHILD_SIZES)
    base = {k: v for k, v in os.environ.items() if k not in KNOBS}
    ran = 0
    for variant in VARIANTS:  # the first failing child ends the test: nothing more is started
        env = dict(base, **{k: str(v) for k, v in variant.items()})
        r = subprocess.run([sys.executable, os.path.join(HERE, "pergate_child.py")] +
                           [str(n) for n in CHILD_SIZES],
                           capture_output=True, text=True, timeout=CHILD_TIMEOUT, env=env)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert lines, (variant, r.returncode, r.stderr[-3000:])
        out = json.loads(lines[-1])
        print(variant, out["cases"], out["worst"])
        assert r.returncode == 0 and out["failures"] == [], (variant, r.returncode,
                                                             out["failures"], r.stderr[-3000:])
        assert out["cases"] == want, (variant, out["cases"], want)
        assert out["worst"] <= pc.TOL
        ran += 1
    assert ran == 7


# ---------------------------------------------------------------- batch stride against the oracle
def _class_circuit(qsim, n, seed):
    """Ry, Rz on every qubit, then every gate type on operands of each class: low/low, low/high and
    high/high pairs, Toffoli with 0, 1 and 2 controls from bit 6, SWAP in ll, lh and hh form."""
    rng = np.random.default_rng(seed)
    ang = lambda: float(rng.uniform(0.1, 2 * math.pi - 0.1))
    c = qsim.Circuit(n)
    for q in range(n):
        c.ry(q, ang()).rz(q, ang())
    lo = [q for q in (0, 2, 3, 5) if q < n]
    if len(lo) < 4:
        lo.append(n - 1)
    hi = sorted({q for q in (6, 7, n - 1) if 6 <= q < n})
    ones = [lo[0], lo[-1]] + hi[:1] + hi[-1:]
    for t in range(11):
        for q in ones:
            c.append(qsim.GateOp(t, [q], ang()))
    pairs = [(lo[0], lo[1]), (lo[2], lo[0]), (lo[3], lo[2])]
    if hi:
        pairs += [(lo[1], hi[0]), (hi[-1], lo[2])]
    if len(hi) >= 2:
        pairs += [(hi[0], hi[-1]), (hi[-1], hi[0])]
    for a, b in pairs:
        for t in (11, 12, 13, 14, 15):
            c.append(qsim.GateOp(t, [a, b], ang()))
    triples = [(lo[0], lo[2], lo[1]), (lo[3], lo[1], lo[0])]
    if hi:
        triples += [(lo[0], lo[1], hi[0]), (lo[2], hi[-1], lo[3]), (hi[0], lo[0], hi[-1])]
    if len(hi) >= 2:
        triples += [(hi[0], hi[-1], lo[1]), (hi[-1], hi[0], lo[3])]
    if len(hi) >= 3:
        triples += [(hi[0], hi[2], hi[1]), (hi[1], hi[2], hi[0])]
    for q in triples:
        c.toffoli(*q)
    return c


@pytest.mark.parametrize("semantics", ["Reference", "Physical"])
@pytest.mark.parametrize("n,B", [(5, 3), (6, 5), (9, 3), (12, 5)])
def test_batched_per_gate_equals_oracle(qsim, oracle, gpu_ready, n, B, semantics):
    """Noise-free BatchedSimulator.run(c, per_gate=True): every trajectory equals the oracle state.
    n < 6: fewer than 64 live lanes and one wave-item per trajectory (items = B, no power of two).
    Under the default (Reference) noise semantics a 12-qubit run takes the gate + noise tile kernel
    instead of launch_op; Physical semantics runs launch_op(..., batch, ...) at every size."""
    c = _class_circuit(qsim, n, 100 * n + B)
    ref = oracle.run_cpu(n, oracle.gates_of(c))
    sim = qsim.BatchedSimulator(n, B, noise=getattr(qsim.BatchedNoise, semantics))
    try:
        sim.run(c, per_gate=True)
        for t in range(B):
            got = sim.getStateVector(t)
            err = max(np.max(np.abs(got.real - ref.real)), np.max(np.abs(got.imag - ref.imag)))
            assert err <= 1e-12, (t, err)
        np.testing.assert_allclose(sim.getAverageProbabilities(), np.abs(ref) ** 2, atol=1e-12, rtol=0)
    finally:
        sim.close()
