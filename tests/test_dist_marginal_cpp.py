"""The C++ tests of the marginal readout of qsim::DistributedSimulator
(tests/cpp_dist_marginal/test_dist_marginal.cpp), run as a child process (ordered before anything
initialises the GPU here).  The values the Python layer computes for the shared 12-qubit case on 8
virtual ranks are obtained in a child process of its own and handed to the harness on its command
line, so no file is shared."""
import os
import subprocess
import sys

import pytest

import marginal_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp_dist_marginal")
BIN = os.path.join(CPP, "build", "test_dist_marginal")

_CHILD = """
import sys
sys.path[:0] = {paths!r}
import numpy as np
import qsim_amd as q
from qsim_amd.dist import DistributedSimulator
import marginal_cases as mc
c = mc.CPP_ENTROPY_CASE
d = DistributedSimulator.virtual(c["n"], 8)
d.run(q.createRandomCircuit(c["n"], c["depth"], c["seed"]))
rho = d.reducedDensityMatrix(c["qubits"])
assert mc.spectrum_is_safe(rho)
print("ENTROPY", repr(mc.entropy_np(rho)))
print("PURITY", repr(d.subsystemPurity(c["qubits"])))
print("MARGINAL", ",".join(repr(float(v)) for v in d.marginalProbabilities([11, 3])))
"""


def _build():
    subprocess.run(["make", "-C", CPP], check=True, capture_output=True, text=True)
    return BIN


def test_cpp_dist_marginal_builds():
    """CPU-side: the new methods compile with g++ alone and link the libraries."""
    assert os.path.exists(_build())


@pytest.mark.gpu
@pytest.mark.subprocess
def test_cpp_dist_marginal_suite():
    exe = _build()
    paths = [os.path.join(ROOT, "cuda-quantum-simulator_amd"), os.path.join(ROOT, "tests")]
    py = subprocess.run([sys.executable, "-s", "-c", _CHILD.format(paths=paths)], capture_output=True, text=True,
                        timeout=120)
    assert py.returncode == 0, py.stdout[-2000:] + py.stderr[-4000:]
    vals = {ln.split()[0]: ln.split()[1] for ln in py.stdout.splitlines()
            if ln.split() and ln.split()[0] in ("ENTROPY", "PURITY", "MARGINAL")}
    print(f"{mc.CPP_ENTROPY_CASE} on 8 virtual ranks by the Python layer: {vals}")
    r = subprocess.run([exe, f"--entropy={vals['ENTROPY']}", f"--purity={vals['PURITY']}",
                        f"--marginal={vals['MARGINAL']}"], capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failed" in r.stdout
