"""The C++ tests of qsim::DistributedSimulator::expectation
(tests/cpp_dist_expectation/test_dist_expectation.cpp), run as a child process (ordered before
anything initialises the GPU here)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp_dist_expectation")
BIN = os.path.join(CPP, "build", "test_dist_expectation")


def _build():
    subprocess.run(["make", "-C", CPP], check=True, capture_output=True, text=True)
    return BIN


def test_cpp_dist_expectation_builds():
    """CPU-side: the header compiles with g++ alone and the method links."""
    assert os.path.exists(_build())


@pytest.mark.gpu
@pytest.mark.subprocess
def test_cpp_dist_expectation_suite():
    exe = _build()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failed" in r.stdout
