"""CPU: the host-only plan of a Pauli-sum expectation value on a sharded state
(qsim_dist_expectation_plan, qsim_amd.dist.expectation_plan): which groups are read inside a shard
and which across ranks, how many half-shard transfers they share, and the error codes — on
hand-made qubit maps for worlds 1, 2 and 8."""
import ctypes

import pytest


def _swap(n, a, b):
    perm = list(range(n))
    perm[a], perm[b] = perm[b], perm[a]
    return perm


def test_symbols_exported(qsim):
    from qsim_amd import _lib
    lib = ctypes.CDLL(_lib.HIP_LIB_PATH)
    for name in ("qsim_dist_expectation", "qsim_dist_expectation_plan"):
        assert hasattr(lib, name), name
    assert _lib.hip.qsim_abi_version() == 2  # additive change
    from qsim_amd.dist import DistributedSimulator
    assert callable(DistributedSimulator.expectation)


@pytest.mark.parametrize("world,n", [(1, 10), (2, 8), (8, 12)])
def test_z_only_sum_is_one_local_group(qsim, world, n):
    from qsim_amd.dist import expectation_plan
    h = qsim.PauliSum(n)
    for q in range(n):                                         # rank positions included
        h.add(0.5 + q, {q: "Z", (q + 1) % n: "Z"})
    h.add(0.25, {})
    for perm in (None, _swap(n, 0, n - 1)):
        p = expectation_plan(n, world, perm, h)
        assert p == {"local_groups": 1, "cross_groups": 0, "transfers": 0, "launches": 1,
                     "bytes_sent_per_rank": 0}


@pytest.mark.parametrize("world,n", [(2, 8), (8, 12)])
def test_x_on_one_rank_qubit(qsim, world, n):
    from qsim_amd.dist import expectation_plan
    L = n - (world.bit_length() - 1)
    # identity map: logical n-1 sits on the top rank position
    p = expectation_plan(n, world, None, qsim.PauliSum(n).add(1.0, {n - 1: "X"}))
    assert p == {"local_groups": 0, "cross_groups": 1, "transfers": 1, "launches": 1,
                 "bytes_sent_per_rank": 8 << L}
    # logical 0 moved to rank position L: X on it crosses, X on the qubit that came local does not
    perm = _swap(n, 0, L)
    p = expectation_plan(n, world, perm, qsim.PauliSum(n).add(1.0, {0: "Y"}))
    assert (p["local_groups"], p["cross_groups"], p["transfers"], p["bytes_sent_per_rank"]) == (0, 1, 1, 8 << L)
    p = expectation_plan(n, world, perm, qsim.PauliSum(n).add(1.0, {L: "X"}))
    assert (p["local_groups"], p["cross_groups"], p["transfers"], p["bytes_sent_per_rank"]) == (1, 0, 0, 0)
    # Z on the rank qubit moves nothing
    p = expectation_plan(n, world, perm, qsim.PauliSum(n).add(1.0, {0: "Z", 1: "X"}))
    assert (p["local_groups"], p["cross_groups"], p["transfers"]) == (1, 0, 0)


def test_thirty_cross_terms_share_six_transfers(qsim):
    from qsim_amd.dist import expectation_plan
    n, world = 12, 8
    L = 9
    # hand-made map: logical 0, 1, 2 on the rank positions 9, 10, 11; logical 11 on the top local
    # position 8
    perm = [9, 10, 11, 0, 1, 2, 3, 4, 5, 6, 7, 8]
    top = 11
    terms = []
    for x_rank in (0b001, 0b110, 0b111):                       # 3 distinct x_rank values
        rank_x = sum(1 << q for q in range(3) if x_rank >> q & 1)
        for k in range(5):                                     # top local position out of x
            terms.append((rank_x | (1 << (3 + k)) if k else rank_x, (k * 37) & 0xFFF, 1.0 + k))
        for k in range(5):                                     # ... and in x
            terms.append((rank_x | 1 << top | (1 << (3 + k)) if k else rank_x | 1 << top, (k * 91) & 0xFFF, 2.0 + k))
    assert len(terms) == 30 and len(set(terms)) == 30
    p = expectation_plan(n, world, perm, terms)
    assert p["local_groups"] == 0
    assert p["cross_groups"] == 30                             # 30 distinct physical x masks
    assert p["transfers"] == 6
    assert p["launches"] == 30
    assert p["bytes_sent_per_rank"] == 6 * (8 << L)
    # the same strings with one x_loc per key: 6 groups, still 6 transfers
    terms = [(sum(1 << q for q in range(3) if xr >> q & 1) | (t << top), z, 1.0)
             for xr in (1, 6, 7) for t in (0, 1) for z in range(5)]
    p = expectation_plan(n, world, perm, terms)
    assert (p["cross_groups"], p["transfers"], p["launches"]) == (6, 6, 6)
    # at world 8 a call never needs more than 14
    every = [(x, 0, 1.0) for x in range(1, 1 << n)]
    p = expectation_plan(n, world, perm, every)
    assert p["transfers"] == 14 and p["cross_groups"] == 7 << L and p["local_groups"] == (1 << L) - 1


def test_world_one_never_crosses(qsim):
    from qsim_amd.dist import expectation_plan
    n = 8
    every = [(x, x >> 1, 1.0) for x in range(1 << n)]
    for perm in (None, list(reversed(range(n)))):
        p = expectation_plan(n, 1, perm, every)
        assert p["cross_groups"] == 0 and p["transfers"] == 0 and p["bytes_sent_per_rank"] == 0
        assert p["local_groups"] == 1 << n


def test_merging_and_launch_count(qsim):
    from qsim_amd.dist import expectation_plan
    n, world = 12, 8
    x = 1 << 11
    # duplicates merge, cancelled coefficients drop, 261 terms of one group take two launches
    terms = [(x, z, 1.0) for z in range(261)] + [(x, 5, 0.5), (1 << 10, 0, 1.0), (1 << 10, 0, -1.0)]
    p = expectation_plan(n, world, None, terms)
    assert (p["cross_groups"], p["transfers"], p["launches"]) == (1, 1, 2)
    assert expectation_plan(n, world, None, [])["launches"] == 0


def test_error_codes(qsim):
    from qsim_amd import _lib
    from qsim_amd.dist import expectation_plan
    c = ctypes
    with pytest.raises(ValueError):
        expectation_plan(8, 3, None, [(1, 0, 1.0)])            # world must be a power of two
    with pytest.raises(ValueError):
        expectation_plan(8, 2, [0, 1, 2], [(1, 0, 1.0)])
    with pytest.raises(ValueError):
        expectation_plan(8, 2, [0, 1, 2, 3, 4, 5, 6, 6], [(1, 0, 1.0)])
    with pytest.raises(ValueError):
        expectation_plan(8, 2, None, qsim.PauliSum(9).add(1.0, {0: "X"}))   # qubit-count mismatch
    outs = [c.c_int(0) for _ in range(4)]
    by = c.c_uint64(0)
    refs = [c.byref(o) for o in outs] + [c.byref(by)]
    t = (_lib.qsim_pauli_term * 1)()
    t[0].x_mask, t[0].z_mask, t[0].coeff = 1 << 8, 0, 1.0      # a qubit index out of range
    assert _lib.hip.qsim_dist_expectation_plan(8, 2, None, t, 1, *refs) == _lib.QSIM_ERR_OUT_OF_RANGE
    t[0].x_mask, t[0].z_mask = 0, 1 << 63
    assert _lib.hip.qsim_dist_expectation_plan(8, 2, None, t, 1, *refs) == _lib.QSIM_ERR_OUT_OF_RANGE
    assert _lib.hip.qsim_dist_expectation_plan(8, 2, None, None, 1, *refs) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert _lib.hip.qsim_dist_expectation_plan(8, 2, None, None, 0, *refs) == _lib.QSIM_OK
    t[0].x_mask, t[0].z_mask = 1, 0
    assert _lib.hip.qsim_dist_expectation_plan(8, 2, None, t, 1, None, *refs[1:]) == _lib.QSIM_ERR_INVALID_ARGUMENT
    # the engine entry without an object: an error, not a crash
    e = c.c_double(0)
    assert _lib.hip.qsim_dist_expectation(None, t, 1, c.byref(e)) == _lib.QSIM_ERR_INVALID_ARGUMENT


def test_method_rejects_qubit_count_mismatch_without_a_device(qsim):
    from qsim_amd.dist import DistributedSimulator
    d = DistributedSimulator.__new__(DistributedSimulator)
    d._h, d._n, d._world, d._rank, d._virtual = ctypes.c_void_p(), 10, 4, 0, True
    with pytest.raises(ValueError, match="qubit count"):
        d.expectation(qsim.PauliSum(9).add(1.0, {0: "Z"}))
