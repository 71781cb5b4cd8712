"""The C++ tests of qsim::DistributedSimulator::gradient
(tests/cpp_dist_gradient/test_dist_gradient.cpp), run as a child process (ordered before anything
initialises the GPU here)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp_dist_gradient")
BIN = os.path.join(CPP, "build", "test_dist_gradient")


def _build():
    subprocess.run(["make", "-C", CPP], check=True, capture_output=True, text=True)
    return BIN


@pytest.mark.gpu
@pytest.mark.subprocess
def test_cpp_dist_gradient_suite():
    exe = _build()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failed" in r.stdout
