"""The C++ tests of qsim::DistributedSimulator's Pauli-string rotations
(tests/cpp_dist_pauli_rotation/test_dist_pauli_rotation.cpp), run as a child process (ordered before
anything initialises the GPU here).  The binary compares with qsim::Simulator itself; its first case
also dumps the value, the gradient and the final amplitudes, which are compared here with the dense
numpy restatement (tests/pauli_rotation_cases.py) at 1e-12 per component and 1e-12 * sum |c|."""
import os
import subprocess

import numpy as np
import pytest

import gradient_cases as gc
import pauli_rotation_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp_dist_pauli_rotation")
BIN = os.path.join(CPP, "build", "test_dist_pauli_rotation")
N = 12


def _build():
    subprocess.run(["make", "-C", CPP], check=True, capture_output=True, text=True)
    return BIN


def _masks(factors):
    x = sum(1 << q for q, p in factors.items() if p in "XY")
    z = sum(1 << q for q, p in factors.items() if p in "YZ")
    return x, z


def _case():
    """The binary's sequence, observable and TFIM chain, restated as (x, z, coeff) masks."""
    seq = []
    for k in range(N):
        if k % 3 == 2:
            seq.append((*_masks({k: "Z", (k + 3) % N: "Z"}), 0.1 * (k + 1)))
        else:
            seq.append((*_masks({k: "XY"[k % 2], (k + 5) % N: "Y", (k + 7) % N: "Z"}), -0.15 * (k + 1)))
    h = []
    for q in range(N):
        h += [(*_masks({q: "Z", (q + 1) % N: "Z"}), 0.3 + 0.05 * q), (*_masks({q: "X"}), -0.2 - 0.01 * q),
              (*_masks({q: "Y", (q + 5) % N: "X"}), 0.15)]
    return seq, h, pc.tfim_terms(N)


def test_cpp_dist_pauli_rotation_builds():
    assert os.path.exists(_build())


@pytest.mark.gpu
@pytest.mark.subprocess
def test_cpp_dist_pauli_rotation_suite(tmp_path):
    exe = _build()
    dump = tmp_path / "dump.txt"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, QSIM_TEST_DUMP=str(dump)))
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failed" in r.stdout
    lines = dump.read_text().split("\n")
    value = float.fromhex(lines[0])
    grad = np.array([float.fromhex(s) for s in lines[1:1 + N]])
    amps = np.array([complex(*(float.fromhex(t) for t in s.split())) for s in lines[1 + N:1 + N + (1 << N)]])
    seq, h, tfim = _case()
    psi = pc.rotate(gc.basis_state(N), *_masks({0: "X", 11: "Y", 5: "Z"}), 0.7)
    psi = pc.run_sequence(psi, pc.trotter_sequence(tfim, 0.4, 2, 2))
    wv, wg = pc.sequence_gradient(psi, seq, h)
    assert np.abs(wg).max() > 1e-3
    bar = gc.bound(h)
    print(f"|dE| = {abs(value - wv):.3e}, max |dgrad| = {np.max(np.abs(grad - wg)):.3e}, bar = {bar:.3e}")
    assert abs(value - wv) <= bar and np.max(np.abs(grad - wg)) <= bar
    want = pc.run_sequence(pc.run_sequence(psi, seq), seq)     # pauliGradient applies seq; then once more
    err = pc.max_component_diff(amps, want)
    print(f"final amplitudes: {err:.3e}")
    assert err < 1e-12
