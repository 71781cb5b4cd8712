"""GPU: the readout kernels of csrc/hip/reduce.hip against numpy at sizes where their grid-stride
loops take more than one trip (k_collapse / k_probabilities: 256 x 32 work-groups of 256 threads,
2^21 threads; k_norm_partial: 2048 work-groups, 2^19 threads), on dense random states uploaded
with fromHost.

  * collapse(bit, result, scale): the kept half is the input times `scale` exactly (one multiply
    per component), the other half exactly zero: every bit at n = 10, bits 0, 6, 22 at n = 23.
  * measureBit: the state after equals the numpy collapse for the returned result, norm 1.
  * getProbabilities at n = 23: re^2 + im^2 within 4 x 2^-52 relative (one rounding per product,
    one for the sum, with or without FMA contraction).
  * probBitZero / getTotalProbability at n = 22 against math.fsum, with (bits 0, 5, 6, 21) and
    without the zero insert.
"""
import math

import numpy as np
import pytest

import pergate_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def psi10():
    psi = pc.random_state(10, 510)
    psi.setflags(write=False)
    return psi


@pytest.fixture(scope="module")
def psi23():
    psi = pc.random_state(23, 523)
    psi.setflags(write=False)
    return psi


@pytest.fixture(scope="module")
def psi22():
    psi = pc.random_state(22, 522)
    psi.setflags(write=False)
    return psi


def _kept(n, bit, result):
    return ((np.arange(1 << n, dtype=np.int64) >> bit) & 1) == result


def _collapsed(psi, kept, scale):
    want = np.zeros_like(psi)
    want.real[kept] = psi.real[kept] * scale
    want.imag[kept] = psi.imag[kept] * scale
    return want


def _check_collapse(sv, psi, n, bit, result):
    kept = _kept(n, bit, result)
    scale = 1.0 / math.sqrt(float(np.sum(np.abs(psi[kept]) ** 2)))
    sv.fromHost(psi)
    sv.collapse(bit, result, scale)
    got = sv.toHost()
    assert np.all(got.real[~kept] == 0.0) and np.all(got.imag[~kept] == 0.0), (bit, result)
    want = _collapsed(psi, kept, scale)
    assert np.array_equal(got[kept], want[kept]), (bit, result, np.max(np.abs(got - want)))


def test_collapse_every_bit(qsim, gpu_ready, psi10):
    sv = qsim.StateVector(10)
    for bit in range(10):
        for result in (0, 1):
            _check_collapse(sv, psi10, 10, bit, result)
    sv.close()


def test_collapse_grid_stride(qsim, gpu_ready, psi23):
    """2^23 amplitudes over 2^21 threads: four trips of k_collapse's loop."""
    sv = qsim.StateVector(23)
    try:
        for bit in (0, 6, 22):
            for result in (0, 1):
                _check_collapse(sv, psi23, 23, bit, result)
    finally:
        sv.close()


def test_measure_bit_collapses_to_returned_result(qsim, gpu_ready, psi10):
    n = 10
    p = np.abs(psi10) ** 2
    sv = qsim.StateVector(n)
    seen = set()
    for seed in range(3):
        sv.setSeed(1000 + seed)
        for bit in range(n):
            sv.fromHost(psi10)
            p0 = sv.probBitZero(bit)
            assert abs(p0 - math.fsum(p[_kept(n, bit, 0)])) <= 1e-12
            result = sv.measureBit(bit)
            assert result in (0, 1)
            seen.add(result)
            pr = p0 if result == 0 else 1.0 - p0
            want = _collapsed(psi10, _kept(n, bit, result), 1.0 / np.sqrt(pr))
            got = sv.toHost()
            err = max(np.max(np.abs(got.real - want.real)), np.max(np.abs(got.imag - want.imag)))
            assert err <= 1e-12, (bit, result, err)
            assert abs(sv.getTotalProbability() - 1.0) <= 1e-12
    assert seen == {0, 1}
    sv.close()


def test_probabilities_grid_stride(qsim, gpu_ready, psi23):
    sv = qsim.StateVector(23)
    try:
        sv.fromHost(psi23)
        got = sv.getProbabilities()
    finally:
        sv.close()
    want = psi23.real * psi23.real + psi23.imag * psi23.imag
    np.testing.assert_allclose(got, want, rtol=4 * 2.0 ** -52, atol=0)


def test_norm_reductions_grid_stride(qsim, gpu_ready, psi22):
    """2^22 (total) and 2^21 (one bit's zero half) elements over k_norm_partial's 2^19 threads."""
    n = 22
    p = psi22.real * psi22.real + psi22.imag * psi22.imag
    sv = qsim.StateVector(n)
    try:
        sv.fromHost(psi22)
        assert abs(sv.getTotalProbability() - math.fsum(p)) <= 1e-12
        for bit in (0, 5, 6, 21):
            assert abs(sv.probBitZero(bit) - math.fsum(p[_kept(n, bit, 0)])) <= 1e-12, bit
    finally:
        sv.close()
