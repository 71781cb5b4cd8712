"""The C++ overlap-matrix tests (tests/cpp_batch_overlap/test_batch_overlap.cpp):
BatchedSimulator::overlapMatrix, kernelMatrix and overlapsWith against the header-only CPU oracle
and their exception types, run as a child process (ordered before anything initialises the GPU
here)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp_batch_overlap")
BIN = os.path.join(CPP, "build", "test_batch_overlap")


def _build():
    subprocess.run(["make", "-C", CPP], check=True, capture_output=True, text=True)
    return BIN


def test_cpp_batch_overlap_builds():
    """CPU-side: the new declarations compile with g++ alone and link the libraries."""
    assert os.path.exists(_build())


@pytest.mark.gpu
@pytest.mark.subprocess
def test_cpp_batch_overlap_suite():
    exe = _build()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failed" in r.stdout
