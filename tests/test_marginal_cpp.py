"""The C++ marginal tests (tests/cpp_marginal/test_marginal.cpp): the readout methods of the C++17
API, run as a child process (ordered before anything initialises the GPU here).  The entropy the
Python layer computes for the shared 12-qubit case is obtained in a child process of its own and
handed to the harness on its command line, so no file is shared."""
import os
import subprocess
import sys

import pytest

import marginal_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp_marginal")
BIN = os.path.join(CPP, "build", "test_marginal")

_CHILD = """
import sys
sys.path[:0] = {paths!r}
import qsim_amd as q
import marginal_cases as mc
c = mc.CPP_ENTROPY_CASE
sim = q.Simulator(c["n"])
sim.run(q.createRandomCircuit(c["n"], c["depth"], c["seed"]))
print("ENTROPY", repr(sim.entanglementEntropy(c["qubits"])))
"""


def _build():
    subprocess.run(["make", "-C", CPP], check=True, capture_output=True, text=True)
    return BIN


def test_cpp_marginal_builds():
    """CPU-side: the new methods compile with g++ alone and link the libraries."""
    assert os.path.exists(_build())


@pytest.mark.gpu
@pytest.mark.subprocess
def test_cpp_marginal_suite():
    exe = _build()
    paths = [os.path.join(ROOT, "cuda-quantum-simulator_amd"), os.path.join(ROOT, "tests")]
    py = subprocess.run([sys.executable, "-s", "-c", _CHILD.format(paths=paths)], capture_output=True, text=True,
                        timeout=120)
    assert py.returncode == 0, py.stdout[-2000:] + py.stderr[-4000:]
    line = [ln for ln in py.stdout.splitlines() if ln.startswith("ENTROPY ")][-1]
    entropy = float(line.split()[1])
    print(f"entropy of {mc.CPP_ENTROPY_CASE} by the Python layer: {entropy!r}")
    r = subprocess.run([exe, f"--entropy={entropy!r}"], capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failed" in r.stdout
