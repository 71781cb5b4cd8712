"""CPU: the host-only plan entries of Pauli-string rotations on the sharded state
(qsim_dist_pauli_rotation_plan, qsim_dist_pauli_gradient_plan; qsim_amd.dist.pauli_rotation_plan,
pauli_gradient_plan) against a small Python restatement of the classification: with L = n -
log2 world local positions a rotation's physical x mask x = x_loc | x_rank << L makes it a phase
rotation (x == 0), a local one (x_rank == 0) or a cross one (x_rank != 0).  Also the entries' error
codes.
"""
import ctypes as c

import numpy as np
import pytest

import gradient_cases as gc
import pauli_rotation_cases as pc

SHAPES = [(2, 8), (4, 10), (8, 12)]
PHASE, LOCAL, CROSS = 0, 1, 2


def to_physical(mask, perm):
    return sum(1 << perm[q] for q in range(len(perm)) if mask >> q & 1)


def classify(n, world, perm, seq):
    """The classes of the sequence's rotations under `perm`, in order."""
    L = n - (world.bit_length() - 1)
    out = []
    for x, _, _ in seq:
        px = to_physical(x, perm)
        out.append(PHASE if px == 0 else LOCAL if px >> L == 0 else CROSS)
    return out


def restated_rotation_plan(n, world, perm, seq):
    L = n - (world.bit_length() - 1)
    cls = classify(n, world, perm, seq)
    runs = [len(r) for r in "".join("p" if k == PHASE else " " for k in cls).split()]
    cross = cls.count(CROSS)
    return {
        "rotations": len(seq), "phase_rotations": cls.count(PHASE), "phase_passes": len(runs),
        "local_rotations": cls.count(LOCAL), "cross_rotations": cross,
        "cross_pure": sum(1 for k, (x, _, _) in zip(cls, seq)
                          if k == CROSS and to_physical(x, perm) & ((1 << L) - 1) == 0),
        "launches": sum((r + 255) // 256 for r in runs) + cls.count(LOCAL) + cross,
        "transfers": cross, "bytes_sent_per_rank": cross * (16 << L)}


def restated_apply_groups(n, world, perm, terms):
    """(local groups, cross groups, transfers) of lambda = H phi: one group per distinct physical x
    mask among the merged terms that do not cancel, one transfer per distinct x_rank != 0."""
    L = n - (world.bit_length() - 1)
    merged = {}
    for x, z, coeff in terms:
        merged[(x, z)] = merged.get((x, z), 0.0) + coeff
    xs = {to_physical(x, perm) for (x, _), coeff in merged.items() if coeff != 0.0}
    return (sum(1 for x in xs if x >> L == 0), sum(1 for x in xs if x >> L), len({x >> L for x in xs if x >> L}))


def random_case(seed, n, count=40):
    rng = np.random.default_rng(seed)
    perm = [int(p) for p in rng.permutation(n)]
    seq = pc.random_rotations(rng, n, count, p_diag=0.4)
    return perm, seq, gc.random_terms(rng, n, 8, 3)


def test_symbols_and_structs(qsim):
    from qsim_amd import _lib
    for name in ("qsim_dist_apply_pauli_rotations", "qsim_dist_pauli_rotation_plan", "qsim_dist_pauli_gradient",
                 "qsim_dist_pauli_gradient_plan"):
        assert hasattr(_lib.hip, name)
    assert c.sizeof(_lib.qsim_dist_pauli_rotation_info) == 8 * 4 + 8
    assert c.sizeof(_lib.qsim_dist_pauli_gradient_info) == 40 + 10 * 4 + 8
    from qsim_amd.dist import DistributedSimulator
    for name in ("applyPauliRotation", "applyPauliRotations", "evolve", "pauliGradient"):
        assert callable(getattr(DistributedSimulator, name))


@pytest.mark.parametrize("world,n", SHAPES)
def test_rotation_plan_matches_the_restatement(qsim, world, n):
    from qsim_amd.dist import pauli_rotation_plan
    seen = set()
    for seed in range(20):
        perm, seq, _ = random_case(seed, n)
        want = restated_rotation_plan(n, world, perm, seq)
        assert pauli_rotation_plan(n, world, perm, seq) == want, seed
        # a PauliSum carries the same sequence
        assert pauli_rotation_plan(n, world, perm, gc.to_pauli_sum(qsim, n, seq)) == want
        seen |= set(classify(n, world, perm, seq))
    assert seen == {PHASE, LOCAL, CROSS}
    # the identity map when perm is None; an empty sequence
    _, seq, _ = random_case(99, n)
    ident = list(range(n))
    assert pauli_rotation_plan(n, world, None, seq) == restated_rotation_plan(n, world, ident, seq)
    assert pauli_rotation_plan(n, world, None, []) == restated_rotation_plan(n, world, ident, [])


@pytest.mark.parametrize("world,n", SHAPES)
def test_phase_runs_merge_as_on_one_gpu(qsim, world, n):
    """Z-only runs are the only thing merged, and exactly as qsim_pauli_rotation_plan merges them:
    x == 0 does not depend on the map, so the passes and launches of the two entries agree."""
    from qsim_amd.dist import pauli_rotation_plan
    from qsim_amd.plan import pauli_rotation_plan as single_plan
    rng = np.random.default_rng(5)
    zrot = lambda: (0, int(rng.integers(0, 1 << n)), float(rng.uniform(-1, 1)))
    xrot = lambda: (int(rng.integers(1, 1 << n)), int(rng.integers(0, 1 << n)), 0.3)
    seq = [zrot() for _ in range(300)] + [xrot()] + [zrot() for _ in range(256)] + [xrot(), xrot(), zrot()]
    perm = [int(p) for p in rng.permutation(n)]
    info = pauli_rotation_plan(n, world, perm, seq)
    assert (info["phase_rotations"], info["phase_passes"]) == (557, 3)
    assert info["launches"] == 2 + 1 + 1 + 3
    passes, launches = single_plan(gc.to_pauli_sum(qsim, n, seq), perm)
    assert passes == info["phase_passes"] + info["local_rotations"] + info["cross_rotations"]
    assert launches == info["launches"]


@pytest.mark.parametrize("world,n", SHAPES)
def test_gradient_plan_matches_the_restatement(qsim, world, n):
    from qsim_amd.dist import pauli_gradient_plan
    L = n - (world.bit_length() - 1)
    firsts = set()
    for seed in range(20):
        perm, seq, terms = random_case(seed, n, 30)
        cls = classify(n, world, perm, seq)
        info = pauli_gradient_plan(n, world, perm, seq, terms)
        fwd = restated_rotation_plan(n, world, perm, seq)
        assert {k[8:]: v for k, v in info.items() if k.startswith("forward_")} == fwd
        assert info["steps"] == len(seq)
        assert [info["steps_phase"], info["steps_local"], info["steps_cross"]] == [cls.count(k) for k in range(3)]
        assert info["first_class"] == cls[0]
        firsts.add(cls[0])
        # phi and lambda cross per cross step; the sequence's first rotation needs phi alone
        assert info["step_transfers"] == 2 * cls.count(CROSS) - (cls[0] == CROSS)
        lg, cg, tr = restated_apply_groups(n, world, perm, terms)
        assert (info["apply_groups_local"], info["apply_groups_cross"], info["apply_transfers"]) == (lg, cg, tr)
        assert info["apply_launches"] == lg + cg
        assert info["bytes_sent_per_rank"] == (fwd["transfers"] + tr + info["step_transfers"]) * (16 << L)
    assert firsts == {PHASE, LOCAL, CROSS}
    # no sweep: H == 0 (no terms, or terms that cancel) or no rotation; the application is still planned
    perm, seq, terms = random_case(3, n, 30)
    fwd = restated_rotation_plan(n, world, perm, seq)
    for h in ([], [(5, 3, 0.4), (5, 3, -0.4)]):
        info = pauli_gradient_plan(n, world, perm, seq, h)
        assert info["steps"] == info["step_transfers"] == info["apply_transfers"] == 0 and info["first_class"] == -1
        assert info["forward_cross_rotations"] == fwd["cross_rotations"]
        assert info["bytes_sent_per_rank"] == fwd["bytes_sent_per_rank"]
    info = pauli_gradient_plan(n, world, perm, [], terms)
    assert info["steps"] == 0 and info["bytes_sent_per_rank"] == 0 and info["first_class"] == -1


def test_world_one_has_no_cross_rotations(qsim):
    from qsim_amd.dist import pauli_gradient_plan, pauli_rotation_plan
    n = 10
    perm, seq, terms = random_case(7, n)
    info = pauli_rotation_plan(n, 1, perm, seq)
    assert info["cross_rotations"] == info["transfers"] == info["bytes_sent_per_rank"] == 0
    assert info["local_rotations"] == sum(1 for x, _, _ in seq if x)
    g = pauli_gradient_plan(n, 1, perm, seq, terms)
    assert g["steps_cross"] == g["step_transfers"] == g["apply_groups_cross"] == g["bytes_sent_per_rank"] == 0


def test_error_codes(qsim):
    from qsim_amd import _lib
    n = 8
    ri, gi = _lib.qsim_dist_pauli_rotation_info(), _lib.qsim_dist_pauli_gradient_info()
    rot = (_lib.qsim_pauli_term * 2)()
    rot[0].x_mask, rot[0].z_mask, rot[0].coeff = 1, 0, 0.3
    rot[1].x_mask, rot[1].z_mask, rot[1].coeff = 0, 3, 0.2
    bad = (_lib.qsim_pauli_term * 2)()
    bad[0].x_mask, bad[0].z_mask, bad[0].coeff = 1, 0, 0.3
    bad[1].x_mask, bad[1].z_mask, bad[1].coeff = 0, 1 << n, 0.2      # a mask bit >= n, at the end
    notperm = (c.c_int32 * n)(0, 1, 2, 3, 4, 5, 6, 6)
    rp, gp = _lib.hip.qsim_dist_pauli_rotation_plan, _lib.hip.qsim_dist_pauli_gradient_plan
    assert rp(n, 2, None, rot, 2, c.byref(ri)) == _lib.QSIM_OK
    assert rp(n, 2, None, bad, 2, c.byref(ri)) == _lib.QSIM_ERR_OUT_OF_RANGE
    assert rp(n, 2, None, None, 2, c.byref(ri)) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert rp(n, 2, None, None, 0, c.byref(ri)) == _lib.QSIM_OK
    assert rp(n, 2, notperm, rot, 2, c.byref(ri)) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert rp(n, 3, None, rot, 2, c.byref(ri)) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert rp(n, 2, None, rot, 2, None) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert gp(n, 2, None, rot, 2, rot, 2, c.byref(gi)) == _lib.QSIM_OK
    assert gp(n, 2, None, bad, 2, rot, 2, c.byref(gi)) == _lib.QSIM_ERR_OUT_OF_RANGE
    assert gp(n, 2, None, rot, 2, bad, 2, c.byref(gi)) == _lib.QSIM_ERR_OUT_OF_RANGE
    assert gp(n, 2, None, None, 2, rot, 2, c.byref(gi)) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert gp(n, 2, None, rot, 2, None, 2, c.byref(gi)) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert gp(n, 2, notperm, rot, 2, rot, 2, c.byref(gi)) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert gp(n, 6, None, rot, 2, rot, 2, c.byref(gi)) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert gp(n, 2, None, rot, 2, rot, 2, None) == _lib.QSIM_ERR_INVALID_ARGUMENT
    # the device entries check their handle before anything else
    v = c.c_double()
    assert _lib.hip.qsim_dist_apply_pauli_rotations(None, rot, 2) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert _lib.hip.qsim_dist_pauli_gradient(None, rot, 2, rot, 2, c.byref(v), None) == _lib.QSIM_ERR_INVALID_ARGUMENT
    from qsim_amd.dist import pauli_rotation_plan
    with pytest.raises(ValueError):
        pauli_rotation_plan(n, 2, [0, 1, 2], [(1, 0, 0.3)])
