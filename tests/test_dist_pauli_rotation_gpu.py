"""GPU: Pauli-string rotations, Trotter evolution and their adjoint gradients on the sharded state
(DistributedSimulator.applyPauliRotation(s) / evolve / pauliGradient; qsim_dist_apply_pauli_rotations,
qsim_dist_pauli_gradient; csrc/hip/dist_pauli_rot.hip, kernels and driver) on virtual ranks.

References: tests/pauli_rotation_cases.py and tests/gradient_cases.py (dense numpy) on the simulator's
own amplitudes read before the call, and the single-GPU Simulator on the same inputs.  Bars: 1e-12
per amplitude component, gc.bound(terms) = 1e-12 * sum |c| on values and gradient entries; every
check of a sequence also holds the numpy-vs-Simulator difference to the bar.  Which classes a case
covers (phase, local, cross; see the plan entry) is asserted through qsim_amd.dist.pauli_rotation_plan
/ pauli_gradient_plan under the map the simulator reports, so a case cannot silently stop covering
a class.
"""
import numpy as np
import pytest

import gradient_cases as gc
import pauli_rotation_cases as pc

pytestmark = pytest.mark.gpu
TOL = 1e-12
PHASE, LOCAL, CROSS = 0, 1, 2

# (world, n): L = 7 (a shard smaller than a work-group), 8, 9 (exactly one), 13 (several)
SHAPES = [(2, 8), (4, 10), (8, 12), (8, 16)]
STARTS = ["fresh", "dense"]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _virtual(world, n):
    from qsim_amd.dist import DistributedSimulator
    return DistributedSimulator.virtual(n, world)


def _start(qsim, world, n, start):
    """fresh: |0..0> under the identity map; dense: two runs of the W-HC circuit, a dense state
    whose map has left the identity."""
    d = _virtual(world, n)
    if start == "dense":
        c = qsim.createRandomHCCircuit(n, 100, 42)
        for _ in range(2):
            d.run(c)
        assert d.perm() != list(range(n))
    return d


def _generic_start(qsim, world, n, start):
    """_start, then a layer of random Rx / Ry / Rz / CRY / CRZ gates.  The W-HC circuit is Clifford:
    on the stabilizer state it leaves (and on |0..0>) a random Pauli string has expectation 0 almost
    surely, so a gradient there is ~0 entry by entry and would not tell a wrong sign from a right one."""
    d = _start(qsim, world, n, start)
    d.run(gc.to_circuit(qsim, n, gc.random_gates(np.random.default_rng(n), n, 4 * n, types=gc.PARAMETRIC)))
    if start == "dense":
        assert d.perm() != list(range(n))
    return d


def _single(qsim, n, psi):
    s = qsim.Simulator(n)
    s.state.fromHost(psi)
    return s


def _diff(got, want, what):
    e = pc.max_component_diff(got, want)
    print(f"{what}: max component diff = {e:.3e}")
    return e


def _check_grad(got, want, terms, what):
    (v, g), (wv, wg) = got, want
    assert g.shape == wg.shape
    bar = gc.bound(terms)
    ev, eg = abs(v - wv), float(np.max(np.abs(g - wg))) if len(g) else 0.0
    print(f"{what}: |dE| = {ev:.3e}, max |dgrad| = {eg:.3e}, bar = {bar:.3e}")
    assert ev <= bar and eg <= bar, what


def _factors(n, x, z):
    f = {}
    for q in range(n):
        xb, zb = x >> q & 1, z >> q & 1
        if xb or zb:
            f[q] = "Y" if xb and zb else ("X" if xb else "Z")
    return f


def _class_cases(n, world, perm):
    """name -> ((x, z) logical masks, class, x_loc == 0), written by PHYSICAL position under perm:
    X / Y / Z factors on chosen local positions (< L) and rank positions (>= L)."""
    g = world.bit_length() - 1
    L = n - g
    inv = {p: q for q, p in enumerate(perm)}
    lx = lambda positions: sum(1 << inv[p] for p in set(positions))  # physical positions -> logical mask
    r0, r1 = L, n - 1                                            # rank positions (the same one when g == 1)
    rng = np.random.default_rng(n)
    wx = int(rng.integers(1, 1 << n)) | lx([r0])
    cases = {
        "identity": ((0, 0), PHASE, False),
        "phase_local_z": ((0, lx([0, 3, L - 1])), PHASE, False),
        "phase_rank_z": ((0, lx([r0])), PHASE, False),
        "phase_mixed_z": ((0, lx([1, L - 1, r0, r1])), PHASE, False),
        "local_x": ((lx([2]), 0), LOCAL, False),
        "local_top_xy": ((lx([0, L - 1]), lx([L - 1, 4])), LOCAL, False),
        "local_x_rank_z": ((lx([1, 5]), lx([r0])), LOCAL, False),
        "local_y_rank_z": ((lx([3]), lx([3, r1, 2])), LOCAL, False),
        "cross_pure_x": ((lx([r0]), 0), CROSS, True),
        "cross_pure_y": ((lx([r1]), lx([r1])), CROSS, True),
        "cross_pure_x_local_z": ((lx([r0]), lx([0, L - 1])), CROSS, True),
        "cross_x_local_x": ((lx([r0, 0]), 0), CROSS, False),
        "cross_y_local_xyz": ((lx([r1, 1, L - 1]), lx([r1, L - 1, 2])), CROSS, False),
        "weight_n_y": (((1 << n) - 1, (1 << n) - 1), CROSS, False),
        "weight_n_mixed": ((wx, ((1 << n) - 1) ^ (wx & 0x5555)), CROSS, False),
    }
    if g >= 2:  # Z and X on different rank positions, X / Y on several
        cases["cross_x_other_rank_z"] = ((lx([r0]), lx([r1])), CROSS, True)
        cases["cross_all_rank_x"] = ((lx(range(L, n)), lx([r0, 6])), CROSS, True)
        cases["cross_xy_two_ranks"] = ((lx([r0, r1, 3]), lx([r1, 3, 0])), CROSS, False)
    return cases


@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("world,n", SHAPES)
def test_class_matrix(qsim, gpu_ready, world, n, start):
    """Single rotations of every class, one after the other on the same state: the sign foldings
    of Y and Z factors on rank positions, x_loc == 0 and != 0, the identity and weight-n strings."""
    from qsim_amd.dist import pauli_rotation_plan
    d = _start(qsim, world, n, start)
    perm = d.perm()
    theta = 0.37
    psi = d.getStateVector()
    for name, ((x, z), cls, pure) in _class_cases(n, world, perm).items():
        info = pauli_rotation_plan(n, world, perm, [(x, z, theta)])
        got_cls = PHASE if info["phase_rotations"] else LOCAL if info["local_rotations"] else CROSS
        assert (got_cls, bool(info["cross_pure"])) == (cls, pure), (name, info)
        theta += 0.41
        want = pc.rotate(psi, x, z, theta)
        one = _single(qsim, n, psi)
        one.applyPauliRotation(_factors(n, x, z), theta)
        assert _diff(one.getStateVector(), want, f"{name}: Simulator vs numpy") < TOL
        d.applyPauliRotation(_factors(n, x, z), theta)
        psi = d.getStateVector()
        assert _diff(psi, want, f"{name}: sharded vs numpy") < TOL, name
        assert d.perm() == perm


def _mixed_rotations(rng, world, n, perm, count):
    """pc.random_rotations, every third one with its x mask cut down to local positions: a random x
    mask over n qubits has a rank position with probability 1 - 1 / world."""
    L = n - (world.bit_length() - 1)
    local = sum(1 << q for q in range(n) if perm[q] < L)
    seq = pc.random_rotations(rng, n, count)
    return [(x & local, z, th) if k % 3 == 1 else (x, z, th) for k, (x, z, th) in enumerate(seq)]


def _random_sequence(world, n, perm):
    """24 rotations with random masks around a Z-only run longer than one phase launch takes (256)."""
    rng = np.random.default_rng(1000 + n)
    seq = _mixed_rotations(rng, world, n, perm, 24)
    run = [(0, int(rng.integers(0, 1 << n)), float(rng.uniform(-0.05, 0.05))) for _ in range(300)]
    return seq[:12] + run + seq[12:]


@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("world,n", SHAPES)
def test_random_sequences(qsim, gpu_ready, world, n, start):
    from qsim_amd.dist import pauli_rotation_plan
    d = _start(qsim, world, n, start)
    perm = d.perm()
    seq = _random_sequence(world, n, perm)
    ps = gc.to_pauli_sum(qsim, n, seq)
    info = pauli_rotation_plan(n, world, perm, ps)
    assert info["phase_passes"] >= 2 and info["local_rotations"] >= 2 and info["cross_rotations"] >= 2, info
    assert info["launches"] > info["phase_passes"] + info["local_rotations"] + info["cross_rotations"]  # the long run
    psi0 = d.getStateVector()
    want = pc.run_sequence(psi0, seq)
    one = _single(qsim, n, psi0)
    one.applyPauliRotations(ps)
    assert _diff(one.getStateVector(), want, "Simulator vs numpy") < TOL
    bytes_before = d.remapBytes()
    d.applyPauliRotations(ps)
    got = d.getStateVector()
    assert _diff(got, want, "sharded vs numpy") < TOL
    assert _diff(got, one.getStateVector(), "sharded vs Simulator") < TOL
    assert d.perm() == perm and d.remapBytes() == bytes_before
    assert abs(d.getTotalProbability() - 1.0) < 1e-12
    # the state still runs: a circuit after the rotations
    gates = gc.random_gates(np.random.default_rng(n), n, 40)
    d.run(gc.to_circuit(qsim, n, gates))
    assert _diff(d.getStateVector(), gc.run(want, n, gates), "run() after the rotations vs numpy") < TOL


@pytest.mark.parametrize("world,n,blocks", [(8, 12, "3"), (8, 12, "1"), (8, 16, "3")])
def test_cross_kernel_takes_several_trips(qsim, gpu_ready, monkeypatch, world, n, blocks):
    """QSIM_PAULI_BLOCKS caps the grid of the cross kernel as of the two single-GPU ones.  (8, 12):
    512 amplitudes per shard; a cap of 3 does not bind (two work-groups), a cap of 1 takes two whole
    trips.  (8, 16): 8192 amplitudes over 768 threads, ten whole trips and a ragged one."""
    from qsim_amd.dist import pauli_rotation_plan
    d = _start(qsim, world, n, "dense")
    seq = _random_sequence(world, n, d.perm())
    ps = gc.to_pauli_sum(qsim, n, seq)
    assert pauli_rotation_plan(n, world, d.perm(), ps)["cross_rotations"] >= 2
    psi0 = d.getStateVector()
    monkeypatch.setenv("QSIM_PAULI_BLOCKS", blocks)
    d.applyPauliRotations(ps)
    got = d.getStateVector()
    monkeypatch.delenv("QSIM_PAULI_BLOCKS")
    assert _diff(got, pc.run_sequence(psi0, seq), f"QSIM_PAULI_BLOCKS={blocks}") < TOL
    # the amplitudes do not depend on the cap
    twin = _start(qsim, world, n, "dense")
    twin.applyPauliRotations(ps)
    assert np.array_equal(_bits(got), _bits(twin.getStateVector()))


def test_world_one_is_the_single_gpu_path(qsim, gpu_ready):
    """A world of one has no cross class and routes phase and local rotations through the same
    kernels with the same arguments as Simulator (n = L, no rank sign): bit for bit."""
    from qsim_amd.dist import DistributedSimulator
    n = 10
    rng = np.random.default_rng(4)
    seq = pc.random_rotations(rng, n, 24)
    terms = gc.random_terms(rng, n, 8, 3)
    ps, h = gc.to_pauli_sum(qsim, n, seq), gc.to_pauli_sum(qsim, n, terms)
    d, one = DistributedSimulator.virtual(n, 1), qsim.Simulator(n)
    d.applyPauliRotations(ps)
    one.applyPauliRotations(ps)
    assert np.array_equal(_bits(d.getStateVector()), _bits(one.getStateVector()))
    assert _diff(d.getStateVector(), pc.run_sequence(gc.basis_state(n), seq), "world 1 vs numpy") < TOL
    _check_grad(d.pauliGradient(ps, h), one.pauliGradient(ps, h), terms, "world 1 vs Simulator.pauliGradient")


# ---- Trotter evolution ----
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("world,n", SHAPES)
def test_evolve_is_the_trotter_sequence(qsim, gpu_ready, world, n, order):
    from qsim_amd.dist import pauli_rotation_plan
    time, steps = 0.9, 2
    terms = pc.tfim_terms(n)
    h = gc.to_pauli_sum(qsim, n, terms)
    d = _start(qsim, world, n, "dense")
    seq = pc.trotter_sequence(terms, time, steps, order)
    info = pauli_rotation_plan(n, world, d.perm(), seq)
    assert info["phase_passes"] >= 1 and info["local_rotations"] >= 1 and info["cross_rotations"] >= 1, info
    psi0 = d.getStateVector()
    want = pc.run_sequence(psi0, seq)
    one = _single(qsim, n, psi0)
    one.evolve(h, time, steps, order)
    assert _diff(one.getStateVector(), want, "Simulator vs numpy") < TOL
    d.evolve(h, time, steps, order)
    assert _diff(d.getStateVector(), want, f"order {order}") < TOL
    for bad in ((0, 1), (1, 3)):
        with pytest.raises(ValueError):
            d.evolve(h, time, *bad)


def test_evolve_of_a_commuting_h_is_exact(qsim, gpu_ready):
    """n = 8 against pc.exact_evolve, the check of the single-GPU test: a commuting H is evolved
    exactly by either order (its strings carry Z factors on the rank position too)."""
    world, n, time = 2, 8, 1.3
    rng = np.random.default_rng(12)
    terms = [(0, int(rng.integers(1, 1 << n)), float(rng.uniform(-1, 1))) for _ in range(12)]
    for steps, order in ((1, 1), (2, 2)):
        d = _start(qsim, world, n, "dense")
        want = pc.exact_evolve(d.getStateVector(), n, terms, time)
        d.evolve(gc.to_pauli_sum(qsim, n, terms), time, steps, order)
        assert _diff(d.getStateVector(), want, f"commuting H, order {order}") < TOL


# ---- pauliGradient ----
def _gradient_case(world, n, perm, first):
    """A random sequence whose first rotation (the sweep's bra-ket-only step) has class `first`."""
    g = world.bit_length() - 1
    L = n - g
    inv = {p: q for q, p in enumerate(perm)}
    lx = lambda positions: sum(1 << inv[p] for p in set(positions))
    rng = np.random.default_rng(500 + 10 * n + first)
    seq = _mixed_rotations(rng, world, n, perm, 16)
    head = {PHASE: (0, lx([0, L]), 0.7), LOCAL: (lx([1, L - 1]), lx([1, n - 1]), -0.6),
            CROSS: (lx([n - 1, 2]), lx([n - 1, L, 0]), 0.9)}[first]
    # H: random strings, one read inside a shard for certain and one read across ranks
    terms = gc.random_terms(rng, n, 8, 3) + [(0, lx([0, L]), -0.25), (lx([n - 1, 1]), lx([L, 1]), 0.35)]
    return [head] + seq, terms


@pytest.mark.parametrize("first", [PHASE, LOCAL, CROSS])
@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("world,n", SHAPES)
def test_gradient(qsim, gpu_ready, world, n, start, first):
    from qsim_amd.dist import pauli_gradient_plan
    d = _generic_start(qsim, world, n, start)
    perm = d.perm()
    seq, terms = _gradient_case(world, n, perm, first)
    ps, h = gc.to_pauli_sum(qsim, n, seq), gc.to_pauli_sum(qsim, n, terms)
    info = pauli_gradient_plan(n, world, perm, ps, h)
    assert info["first_class"] == first and info["steps"] == len(seq)
    assert info["steps_phase"] >= 2 and info["steps_local"] >= 2 and info["steps_cross"] >= 2, info
    assert info["apply_groups_cross"] >= 1 and info["apply_groups_local"] >= 1, info
    psi0 = d.getStateVector()
    want = pc.sequence_gradient(psi0, seq, terms)
    assert np.abs(want[1]).max() > 1e-3
    ref = _single(qsim, n, psi0).pauliGradient(ps, h)
    _check_grad(ref, want, terms, "Simulator vs numpy")
    got = d.pauliGradient(ps, h)
    _check_grad(got, want, terms, "sharded vs numpy")
    _check_grad(got, ref, terms, "sharded vs Simulator")
    assert d.perm() == perm
    assert _diff(d.getStateVector(), pc.run_sequence(psi0, seq), "state after the call") < TOL


@pytest.mark.parametrize("world,n", [(4, 10), (8, 16)])
def test_gradient_state_after_and_reproducible(qsim, gpu_ready, world, n):
    d, twin, d2 = (_generic_start(qsim, world, n, "dense") for _ in range(3))
    seq, terms = _gradient_case(world, n, d.perm(), CROSS)
    ps, h = gc.to_pauli_sum(qsim, n, seq), gc.to_pauli_sum(qsim, n, terms)
    a = d.pauliGradient(ps, h)
    twin.applyPauliRotations(ps)
    assert d.perm() == twin.perm() and d.remapBytes() == twin.remapBytes()
    assert np.array_equal(_bits(d.getStateVector()), _bits(twin.getStateVector()))
    # two calls from the same state: bitwise-equal results
    b = d2.pauliGradient(ps, h)
    assert a[0] == b[0] and np.array_equal(_bits(a[1]), _bits(b[1]))


def test_gradient_edges_and_memory(qsim, gpu_ready):
    world, n = 4, 10
    d = _generic_start(qsim, world, n, "dense")
    seq, terms = _gradient_case(world, n, d.perm(), LOCAL)
    ps, h = gc.to_pauli_sum(qsim, n, seq), gc.to_pauli_sum(qsim, n, terms)
    psi0 = d.getStateVector()
    assert d.gradientMemoryBytes() == 0
    # count == 0: <H> of the state as it is, nothing applied, nothing allocated
    v, g = d.pauliGradient(qsim.PauliSum(n), h)
    assert g.shape == (0,) and v == d.expectation(h) and abs(v - gc.expectation(psi0, terms)) <= gc.bound(terms)
    assert np.array_equal(_bits(d.getStateVector()), _bits(psi0)) and d.gradientMemoryBytes() == 0
    # nterms == 0 and H == 0: zeros, no sweep, no allocation, and the sequence was still applied
    rotated = pc.run_sequence(psi0, seq)
    for zero in (qsim.PauliSum(n), gc.to_pauli_sum(qsim, n, [(5, 3, 0.4), (5, 3, -0.4)])):
        z = _generic_start(qsim, world, n, "dense")
        v, g = z.pauliGradient(ps, zero)
        assert v == 0.0 and list(g) == [0.0] * len(seq) and z.gradientMemoryBytes() == 0
        assert _diff(z.getStateVector(), rotated, "H = 0: the rotated state") < TOL
    d.pauliGradient(ps, h)
    assert d.gradientMemoryBytes() == 2 * 16 * (1 << n)          # two shards per rank, all ranks here
    d.releaseGradientBuffers()
    assert d.gradientMemoryBytes() == 0
    # a second call after the release, from where the first one ended
    psi1 = d.getStateVector()
    _check_grad(d.pauliGradient(ps, h), pc.sequence_gradient(psi1, seq, terms), terms, "after release")
    assert d.gradientMemoryBytes() == 2 * 16 * (1 << n)


def test_after_a_circuit_gradient_and_expectation(qsim, gpu_ready):
    """The rotation sweep shares the work shards and the staging buffers with gradient() and
    expectation(): calls of the three in turn do not disturb one another."""
    world, n = 4, 10
    d = _start(qsim, world, n, "dense")
    gates, cterms = gc.random_case(0, n)
    d.gradient(gc.to_circuit(qsim, n, gates), gc.to_pauli_sum(qsim, n, cterms))
    seq, terms = _gradient_case(world, n, d.perm(), CROSS)
    ps, h = gc.to_pauli_sum(qsim, n, seq), gc.to_pauli_sum(qsim, n, terms)
    psi0 = d.getStateVector()
    got = d.pauliGradient(ps, h)
    _check_grad(got, pc.sequence_gradient(psi0, seq, terms), terms, "after gradient()")
    assert got[0] == d.expectation(h)


# ---- errors: raised before anything is applied, on Simulator's exception types ----
def test_errors_leave_the_state_unchanged(qsim, gpu_ready):
    import ctypes
    from qsim_amd import _lib
    world, n = 4, 10
    d = _start(qsim, world, n, "dense")
    before, perm = d.getStateVector(), d.perm()
    h = gc.to_pauli_sum(qsim, n, [(0, 3, 1.0)])
    with pytest.raises(IndexError):
        d.applyPauliRotation({0: "X", n: "Z"}, 0.3)
    with pytest.raises(IndexError):
        d.applyPauliRotation({-1: "X"}, 0.3)
    with pytest.raises(ValueError):
        d.applyPauliRotations(qsim.PauliSum(n - 1).add(0.3, {0: "X"}))
    with pytest.raises(ValueError):
        d.pauliGradient(qsim.PauliSum(n + 1).add(0.3, {0: "X"}), h)
    with pytest.raises(ValueError):
        d.pauliGradient(qsim.PauliSum(n).add(0.3, {0: "X"}), qsim.PauliSum(n - 1))
    with pytest.raises(ValueError):
        d.evolve(qsim.PauliSum(n - 1).add(1.0, {0: "Z"}), 1.0)
    # the ABI itself: a bad mask at the END of a sequence is found before the first launch or post
    rots = (_lib.qsim_pauli_term * 3)()
    for k, (x, z, c) in enumerate([((1 << n) - 1, 0, 0.4), (0, 5, 0.3), (1 << n, 0, 0.2)]):
        rots[k].x_mask, rots[k].z_mask, rots[k].coeff = x, z, c
    t, nt = h.to_abi(n)
    v, g = ctypes.c_double(), (ctypes.c_double * 3)()
    f, fg = _lib.hip.qsim_dist_apply_pauli_rotations, _lib.hip.qsim_dist_pauli_gradient
    assert f(d._h, rots, 3) == _lib.QSIM_ERR_OUT_OF_RANGE
    assert f(d._h, None, 3) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert f(d._h, None, 0) == _lib.QSIM_OK
    assert fg(d._h, rots, 3, t, nt, ctypes.byref(v), g) == _lib.QSIM_ERR_OUT_OF_RANGE
    assert fg(d._h, rots, 2, rots, 3, ctypes.byref(v), g) == _lib.QSIM_ERR_OUT_OF_RANGE   # the observable's mask
    assert fg(d._h, rots, 2, t, nt, None, g) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert fg(d._h, rots, 2, t, nt, ctypes.byref(v), None) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert fg(d._h, None, 2, t, nt, ctypes.byref(v), g) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert fg(d._h, rots, 2, None, nt, ctypes.byref(v), g) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert np.array_equal(_bits(d.getStateVector()), _bits(before)) and d.perm() == perm


def test_profile_names(qsim, gpu_ready):
    world, n = 4, 10
    d = _start(qsim, world, n, "dense")
    seq, terms = _gradient_case(world, n, d.perm(), CROSS)
    d.profile(True)
    d.pauliGradient(gc.to_pauli_sum(qsim, n, seq), gc.to_pauli_sum(qsim, n, terms))
    stats = {s["name"]: s for s in d.profileStats()}
    for name in ("dist_pauli_rot", "pauli_rot", "pauli_phase", "pauli_adjoint_step", "pauli_apply"):
        assert name in stats and stats[name]["launches"] > 0 and stats[name]["alg_bytes"] > 0, (name, sorted(stats))
