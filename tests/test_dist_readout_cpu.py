"""CPU: the ABI surface and the host-only decisions of the sharded readout (sample, measure,
probabilities): the new symbols, the sampler's chunk size and localization set for hand-made
qubit maps (qsim_dist_sample_plan), and argument checks that need no device."""
import ctypes

import pytest


NEW_SYMBOLS = ["qsim_dist_bcast", "qsim_dist_probabilities", "qsim_dist_sample", "qsim_dist_collapse",
               "qsim_dist_measure", "qsim_dist_sample_plan"]


def test_new_symbols_exported(qsim):
    from qsim_amd import _lib
    lib = ctypes.CDLL(_lib.HIP_LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert _lib.hip.qsim_abi_version() == 2  # additive change


def test_sample_plan_identity(qsim):
    from qsim_amd.dist import sample_plan
    for n, world in [(8, 2), (10, 4), (12, 8), (16, 8), (20, 2), (30, 8), (14, 1)]:
        L = n - (world.bit_length() - 1)
        c, mask = sample_plan(n, world, list(range(n)))
        assert c == min(12, L), (n, world)
        assert mask == 0, (n, world)


def test_sample_plan_low_qubit_on_rank_position(qsim):
    from qsim_amd.dist import sample_plan
    # 16 qubits on 8 ranks: L = 13, c = 12, rank positions 13..15
    perm = list(range(16))
    perm[3], perm[14] = perm[14], perm[3]      # logical 3 on a rank position
    assert sample_plan(16, 8, perm) == (12, 1 << 3)
    perm[0], perm[15] = perm[15], perm[0]      # and logical 0
    assert sample_plan(16, 8, perm) == (12, (1 << 3) | 1)
    # a HIGH logical qubit (>= c) on a rank position needs no remap, wherever the low ones sit
    perm = list(range(16))
    perm[12], perm[13] = perm[13], perm[12]
    perm[0], perm[11] = perm[11], perm[0]
    assert sample_plan(16, 8, perm) == (12, 0)


def test_sample_plan_small_shards(qsim):
    from qsim_amd.dist import sample_plan
    # L < 12: the chunk is the whole shard's worth of low logical qubits, c = L
    perm = list(range(10))
    assert sample_plan(10, 4, perm) == (8, 0)
    perm[7], perm[8] = perm[8], perm[7]        # logical 7 < c on rank position 8
    assert sample_plan(10, 4, perm) == (8, 1 << 7)
    perm = list(range(12))
    perm[9], perm[2] = perm[2], perm[9]        # 12 qubits / 8 ranks: L = c = 9; logical 2 -> pos 9
    assert sample_plan(12, 8, perm) == (9, 1 << 2)


def test_sample_plan_rejects_bad_maps(qsim):
    from qsim_amd.dist import sample_plan
    with pytest.raises(ValueError):
        sample_plan(8, 2, [0, 1, 2, 3, 4, 5, 6, 6])
    with pytest.raises(ValueError):
        sample_plan(8, 2, [0, 1, 2, 3, 4, 5, 6, 8])
    with pytest.raises(ValueError):
        sample_plan(8, 2, [0, 1, 2])
    with pytest.raises(ValueError):
        sample_plan(8, 3, list(range(8)))      # world must be a power of two


def test_methods_reject_bad_arguments_without_a_device(qsim):
    """The argument checks of StateVector, made before any engine call: an object without an
    engine handle is enough to reach them."""
    from qsim_amd.dist import DistributedSimulator
    d = DistributedSimulator.__new__(DistributedSimulator)
    d._h, d._n, d._world, d._rank, d._virtual = ctypes.c_void_p(), 10, 4, 0, True
    with pytest.raises(ValueError, match="n_shots must be positive"):
        d.sample(0)
    with pytest.raises(ValueError, match="n_shots must be positive"):
        d.sample(-3)
    with pytest.raises(ValueError, match="n_shots must be positive"):
        d.sampleWith([])
    for bad in (-1, 10):
        with pytest.raises(ValueError, match="out of range"):
            d.measureBit(bad)
        with pytest.raises(ValueError, match="out of range"):
            d.measureQubit(bad)
    d.setSeed(7)
    assert d._rng is not None


def test_null_handle_is_an_error_not_a_crash(qsim):
    from qsim_amd import _lib
    r = ctypes.c_int(0)
    assert _lib.hip.qsim_dist_measure(None, 0, 0.5, ctypes.byref(r)) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert _lib.hip.qsim_dist_collapse(None, 0, 0, 1.0) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert _lib.hip.qsim_dist_probabilities(None, None) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert _lib.hip.qsim_dist_bcast(None, None, 0) == _lib.QSIM_ERR_INVALID_ARGUMENT
