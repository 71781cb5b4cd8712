"""The C++ density-matrix subset-reader tests (tests/cpp_dm_marginal/test_dm_marginal.cpp):
marginalProbabilities, reducedDensityMatrix, subsystemPurity, subsystemEntropy and fidelity of
DensityMatrix / DensityMatrixSimulator in the C++17 API, run as a child process (ordered before
anything initialises the GPU here)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp_dm_marginal")
BIN = os.path.join(CPP, "build", "test_dm_marginal")


def _build():
    subprocess.run(["make", "-C", CPP], check=True, capture_output=True, text=True)
    return BIN


def test_cpp_dm_marginal_builds():
    """CPU-side: the new methods compile with g++ alone and link the libraries."""
    assert os.path.exists(_build())


@pytest.mark.gpu
@pytest.mark.subprocess
def test_cpp_dm_marginal_suite():
    exe = _build()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failed" in r.stdout
