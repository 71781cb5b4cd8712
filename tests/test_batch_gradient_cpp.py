"""The C++ sweep-gradient tests (tests/cpp_batch_gradient/test_batch_gradient.cpp):
BatchedSimulator::gradientSweep against the C ABI call it wraps (bitwise), a closed form and the
exception types of runSweep, run as a child process (ordered before anything initialises the GPU
here)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp_batch_gradient")
BIN = os.path.join(CPP, "build", "test_batch_gradient")


def _build():
    subprocess.run(["make", "-C", CPP], check=True, capture_output=True, text=True)
    return BIN


def test_cpp_batch_gradient_builds():
    """CPU-side: the new declarations compile with g++ alone and link the libraries."""
    assert os.path.exists(_build())


@pytest.mark.gpu
@pytest.mark.subprocess
def test_cpp_batch_gradient_suite():
    exe = _build()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failed" in r.stdout
