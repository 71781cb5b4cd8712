"""GPU: adjoint-method gradients on the sharded state (DistributedSimulator.gradient,
qsim_dist_gradient; csrc/hip/dist_adjoint.hip, kernels and driver) on virtual ranks.

Reference: tests/gradient_cases.py (dense numpy adjoint sweep) on the simulator's own amplitudes
read before the call, and Simulator.gradient on the same inputs; bar gc.bound(terms) = 1e-12 *
sum |c| on the value and on every gradient entry, as tests/test_gradient_gpu.py.  Which classes of
the sweep a case covers is asserted through the host-only plan entry (qsim_amd.dist.gradient_plan)
under the map the simulator reports, so a case cannot silently stop covering a class.  The seeds
were found with that entry on the CPU.
"""
import numpy as np
import pytest

import gradient_cases as gc

pytestmark = pytest.mark.gpu

# (world, n): L = 7 (a shard smaller than a work-group), 8, 9 (exactly one), 13 (several)
SHAPES = [(2, 8), (4, 10), (8, 12), (8, 16)]
# rotations-only circuits (seed, gate count) whose sweep from the dense start covers every class
MATRIX = {(2, 8): (1039, 48), (4, 10): (1022, 48), (8, 12): (1005, 48), (8, 16): (1024, 72)}
# gc.random_case seeds whose sweep has a remapping segment from |0..0> and from the dense start
RANDOM = {(2, 8): [1, 2, 8, 9], (4, 10): [0, 1, 2, 3], (8, 12): [0, 1, 2, 3], (8, 16): [2, 3, 5, 6]}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _virtual(world, n, **kw):
    from qsim_amd.dist import DistributedSimulator
    return DistributedSimulator.virtual(n, world, **kw)


def _dense(qsim, world, n, **kw):
    """Two runs of the W-HC circuit: a dense state whose map has left the identity."""
    d = _virtual(world, n, **kw)
    c = qsim.createRandomHCCircuit(n, 100, 42)
    for _ in range(2):
        d.run(c)
    assert d.perm() != list(range(n))
    return d


_REF = {}


def _reference(key, psi0, n, gates, terms):
    """numpy value and gradient; computed once per case, read-only."""
    if key not in _REF:
        v, g = gc.adjoint_gradient(psi0, n, gates, terms)
        g.setflags(write=False)
        _REF[key] = (v, g)
    return _REF[key]


def _check(got, want, terms, what):
    v, g = got
    wv, wg = want
    bar = gc.bound(terms)
    ev, eg = abs(v - wv), float(np.max(np.abs(g - wg))) if len(g) else 0.0
    print(f"{what}: |dE| = {ev:.3e}, max |dgrad| = {eg:.3e}, bar = {bar:.3e}")
    assert ev <= bar and eg <= bar, what


def _single(qsim, n, psi0, gates, terms, fused=True):
    s = qsim.Simulator(n)
    s.state.fromHost(psi0)
    v, g = s.gradient(gc.to_circuit(qsim, n, gates), gc.to_pauli_sum(qsim, n, terms),
                      qsim.RunMode.Fused if fused else qsim.RunMode.PerGate)
    return v, g


def _matrix_case(n, world):
    seed, count = MATRIX[(world, n)]
    rng = np.random.default_rng(seed)
    gates = gc.random_gates(rng, n, count, types=gc.PARAMETRIC)
    return gates, gc.random_terms(rng, n, 8, 3)


@pytest.mark.parametrize("world,n", SHAPES)
def test_step_matrix(qsim, gpu_ready, monkeypatch, world, n):
    from qsim_amd.dist import gradient_plan
    gates, terms = _matrix_case(n, world)
    c, h = gc.to_circuit(qsim, n, gates), gc.to_pauli_sum(qsim, n, terms)
    d = _dense(qsim, world, n)
    info = gradient_plan(c, world, h, d.perm())
    need = ["steps_local", "steps_local_crank", "steps_diag", "steps_cross", "cross_rx", "cross_ry", "cross_cry",
            "local_ctrl_below", "local_ctrl_above"]
    if world >= 4:  # (one rank position cannot hold both the target and the control)
        need += ["steps_diag_crank", "steps_cross_crank"]
    assert all(info[k] > 0 for k in need), info
    assert info["segments"] == 0 and info["params"] == len(gates)
    psi0 = d.getStateVector()
    want = _reference(("matrix", world, n), psi0, n, gates, terms)
    monkeypatch.delenv("QSIM_ADJOINT_FUSED", raising=False)
    got = d.gradient(c, h)
    assert d.perm() == info["perm_after_run"]
    _check(got, want, terms, "fused steps")
    _check(got, _single(qsim, n, psi0, gates, terms), terms, "vs Simulator.gradient")
    # the same call with the local class composed from a reduction and two per-gate launches
    d2 = _dense(qsim, world, n)
    monkeypatch.setenv("QSIM_ADJOINT_FUSED", "0")
    got0 = d2.gradient(c, h)
    _check(got0, want, terms, "QSIM_ADJOINT_FUSED=0")
    # the cross classes never read the variable: bitwise equal
    L = n - (world.bit_length() - 1)
    perm = info["perm_after_run"]
    cross = [k for k, (t, q, _) in enumerate(gates) if perm[q[-1]] >= L]
    assert cross and np.array_equal(_bits(got[1][cross]), _bits(got0[1][cross]))


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("start", ["fresh", "dense"])
@pytest.mark.parametrize("world,n", SHAPES)
def test_random_circuits(qsim, gpu_ready, world, n, start, fused):
    from qsim_amd.dist import gradient_plan
    assert {t for seed in RANDOM[(world, n)] for t, _, _ in gc.random_case(seed, n)[0]} == set(range(17))
    for seed in RANDOM[(world, n)]:
        gates, terms = gc.random_case(seed, n)
        c, h = gc.to_circuit(qsim, n, gates), gc.to_pauli_sum(qsim, n, terms)
        d = _dense(qsim, world, n) if start == "dense" else _virtual(world, n)
        # (states this small are never relabeled on their first run: the plan holds for |0..0> too)
        info = gradient_plan(c, world, h, d.perm())
        assert info["remap_segments"] >= 1, info
        psi0 = d.getStateVector()
        want = _reference(("random", world, n, seed, start), psi0, n, gates, terms)
        got = d.gradient(c, h, fused=fused)
        assert d.perm() == info["perm_after_run"]
        _check(got, want, terms, f"seed {seed} {start} fused={fused}")
        if fused:
            _check(got, _single(qsim, n, psi0, gates, terms), terms, f"seed {seed} vs Simulator.gradient")


@pytest.mark.parametrize("world,n", SHAPES)
def test_observable_coverage(qsim, gpu_ready, world, n):
    """A mixed H: local and cross groups, two cross groups sharing one transfer, and a group of more
    than kExpectTerms (256) terms on an x mask with a rank position."""
    from qsim_amd.dist import gradient_plan
    g = world.bit_length() - 1
    L = n - g
    d = _dense(qsim, world, n)
    gates, _ = gc.random_case(3, n)
    c = gc.to_circuit(qsim, n, gates)
    # the sweep reads H under the map AFTER the forward run: choose the strings by position there
    pa = gradient_plan(c, world, [(0, 1, 1.0)], d.perm())["perm_after_run"]
    inv = {p: q for q, p in enumerate(pa)}
    lx = lambda positions: sum(1 << inv[p] for p in positions)   # physical positions -> logical mask
    rng = np.random.default_rng(77)
    terms = [(0, int(rng.integers(1, 1 << n)), 0.5), (lx([1]), lx([1, L]), -0.3), (lx([0, 3]), 0, 0.2)]
    # (8 qubits have only 256 z masks: one x mask cannot hold more than kExpectTerms distinct strings there)
    big = min(300, 1 << n)
    terms += [(lx([L]), int(z), float(rng.uniform(-1, 1)) / 64) for z in rng.choice(1 << n, big, replace=False)]
    terms += [(lx([L, 2]), lx([2, n - 1]), 0.7)]                 # same x_rank as the big group: one transfer
    if g >= 2:
        terms += [(lx([L, n - 1, 1]), lx([L]), -0.4)]
    h = gc.to_pauli_sum(qsim, n, terms)
    info = gradient_plan(c, world, h, d.perm())
    assert info["perm_after_run"] == pa
    assert info["apply_groups_local"] == 3 and info["apply_groups_cross"] == (3 if g >= 2 else 2)
    assert info["apply_transfers"] == (2 if g >= 2 else 1)       # two groups share the transfer of x_rank = 1
    assert info["apply_launches"] == info["apply_groups_local"] + info["apply_groups_cross"] + (big > 256)
    psi0 = d.getStateVector()
    got = d.gradient(c, h)
    _check(got, gc.adjoint_gradient(psi0, n, gates, terms), terms, "mixed H")


@pytest.mark.parametrize("world,n", [(4, 10), (8, 16)])
def test_state_after_and_reproducible(qsim, oracle, gpu_ready, world, n):
    gates, terms = gc.random_case(RANDOM[(world, n)][0], n)
    c, h = gc.to_circuit(qsim, n, gates), gc.to_pauli_sum(qsim, n, terms)
    d, twin = _dense(qsim, world, n), _dense(qsim, world, n)
    a = d.gradient(c, h)
    twin.run(c)
    assert d.perm() == twin.perm()
    assert np.array_equal(_bits(d.getStateVector()), _bits(twin.getStateVector()))
    assert (d.overlappedRemaps(), d.fusedRemaps(), d.remapBytes()) == (
        twin.overlappedRemaps(), twin.fusedRemaps(), twin.remapBytes())
    # two calls from the same state: bitwise-equal results
    d2 = _dense(qsim, world, n)
    b = d2.gradient(c, h)
    assert a[0] == b[0] and np.array_equal(_bits(a[1]), _bits(b[1]))
    # the state still runs
    hc = qsim.createRandomHCCircuit(n, 100, 42)
    d.run(hc)
    ref = oracle.run_cpu(n, oracle.gates_of(hc) * 2 + oracle.gates_of(c) + oracle.gates_of(hc))
    assert np.max(np.abs(d.getStateVector() - ref)) < 1e-12


def test_virtual_ranks_over_rccl(qsim, gpu_ready):
    world, n = 4, 14
    gates, terms = gc.random_case(1, n)
    c, h = gc.to_circuit(qsim, n, gates), gc.to_pauli_sum(qsim, n, terms)
    from qsim_amd.dist import gradient_plan
    d = _dense(qsim, world, n, rccl=True)
    info = gradient_plan(c, world, h, d.perm())
    assert info["steps_cross"] + info["steps_cross_crank"] >= 1 and info["segment_remaps"] >= 1, info
    psi0 = d.getStateVector()
    _check(d.gradient(c, h), gc.adjoint_gradient(psi0, n, gates, terms), terms, "virtual ranks over RCCL")


def test_world_one(qsim, gpu_ready):
    from qsim_amd.dist import DistributedSimulator, gradient_plan
    n = 10
    gates, terms = gc.random_case(4, n)
    c, h = gc.to_circuit(qsim, n, gates), gc.to_pauli_sum(qsim, n, terms)
    info = gradient_plan(c, 1, h)
    assert info["steps_local"] == info["params"] > 0 and info["bytes_sent_per_rank"] == 0
    assert info["apply_groups_cross"] == info["step_transfers"] == info["segment_remaps"] == 0
    d = DistributedSimulator.virtual(n, 1)       # no staging buffers exist in a world of one
    got = d.gradient(c, h)
    _check(got, _single(qsim, n, gc.basis_state(n), gates, terms), terms, "world 1 vs Simulator.gradient")


def test_after_carried_runs(qsim, gpu_ready, monkeypatch):
    """QSIM_DIST_CARRY=1 runs at (8, 20) may leave their last step pending: the call flushes it."""
    world, n = 8, 20
    monkeypatch.setenv("QSIM_DIST_CARRY", "1")
    d = _virtual(world, n)
    hc = qsim.createRandomHCCircuit(n, 100, 42)
    for _ in range(3):
        d.run(hc)
    th = 0.1 + 0.05 * np.arange(n)
    gates = [(gc.RY, [q], float(th[q])) for q in range(n)] + [(gc.CZ, [q, q + 1], 0.0) for q in range(n - 1)]
    terms = [(0, 1 << q, 1.0) for q in range(n)]
    twin = _virtual(world, n)
    for _ in range(3):
        twin.run(hc)
    psi0 = twin.getStateVector()                 # (a reader: flushes the twin's pending step)
    got = d.gradient(gc.to_circuit(qsim, n, gates), gc.to_pauli_sum(qsim, n, terms))
    _check(got, gc.adjoint_gradient(psi0, n, gates, terms), terms, "after carried runs")


def test_memory(qsim, gpu_ready):
    world, n = 4, 10
    gates, terms = gc.random_case(0, n)
    c, h = gc.to_circuit(qsim, n, gates), gc.to_pauli_sum(qsim, n, terms)
    d = _dense(qsim, world, n)
    assert d.gradientMemoryBytes() == 0
    z = _dense(qsim, world, n)
    zero = z.gradient(c, qsim.PauliSum(n))       # no terms: the run alone, no sweep, no allocation
    assert zero[0] == 0.0 and not zero[1].any() and z.gradientMemoryBytes() == 0
    a = d.gradient(c, h)
    assert d.gradientMemoryBytes() == 2 * 16 * (1 << n)          # two shards per rank, all ranks here
    d.releaseGradientBuffers()
    assert d.gradientMemoryBytes() == 0
    d.releaseGradientBuffers()                   # nothing to free: fine
    # a second call after the release works: the same circuit again, from where the first call ended
    psi1 = d.getStateVector()
    b = d.gradient(c, h)
    assert d.gradientMemoryBytes() == 2 * 16 * (1 << n)
    _check(b, gc.adjoint_gradient(psi1, n, gates, terms), terms, "after release")


def test_errors_and_edges(qsim, gpu_ready):
    import ctypes
    from qsim_amd import _lib
    world, n = 4, 10
    d = _dense(qsim, world, n)
    gates, terms = gc.random_case(0, n)
    c, h = gc.to_circuit(qsim, n, gates), gc.to_pauli_sum(qsim, n, terms)
    arr, cnt = c.to_abi()
    t, nt = h.to_abi(n)
    v, g = ctypes.c_double(), (ctypes.c_double * cnt)()
    f = _lib.hip.qsim_dist_gradient
    before = d.getStateVector()
    assert f(d._h, arr, cnt, t, nt, 1, None, g) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert f(d._h, arr, cnt, t, nt, 1, ctypes.byref(v), None) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert f(d._h, None, cnt, t, nt, 1, ctypes.byref(v), g) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert f(d._h, arr, cnt, None, nt, 1, ctypes.byref(v), g) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert f(None, arr, cnt, t, nt, 1, ctypes.byref(v), g) == _lib.QSIM_ERR_INVALID_ARGUMENT
    bad = (_lib.qsim_pauli_term * 1)()
    bad[0].x_mask, bad[0].z_mask, bad[0].coeff = 1 << n, 0, 1.0
    assert f(d._h, arr, cnt, bad, 1, 1, ctypes.byref(v), g) == _lib.QSIM_ERR_OUT_OF_RANGE
    badg = (_lib.qsim_gate * 1)()
    badg[0].type, badg[0].nqubits, badg[0].qubits[0] = 8, 1, n  # Rx on qubit n
    run_rc = _lib.hip.qsim_dist_run(d._h, badg, 1, 1)
    assert run_rc != _lib.QSIM_OK and f(d._h, badg, 1, t, nt, 1, ctypes.byref(v), g) == run_rc
    assert np.array_equal(_bits(d.getStateVector()), _bits(before))   # no failed call ran anything
    with pytest.raises(ValueError):
        d.gradient(qsim.Circuit(n + 1), h)
    # count == 0: the value of the state as it is
    val, grad = d.gradient(qsim.Circuit(n), h)
    assert len(grad) == 0 and abs(val - gc.expectation(before, terms)) <= gc.bound(terms)
    assert val == d.expectation(h)


def test_profile_names(qsim, gpu_ready):
    world, n = 4, 10
    gates, terms = _matrix_case(n, world)
    d = _dense(qsim, world, n)
    d.profile(True)
    d.gradient(gc.to_circuit(qsim, n, gates), gc.to_pauli_sum(qsim, n, terms))
    stats = {s["name"]: s for s in d.profileStats()}
    for name in ("dist_adjoint_step", "dist_adjoint_diag", "pauli_apply", "adjoint_step"):
        assert name in stats and stats[name]["launches"] > 0 and stats[name]["alg_bytes"] > 0, (name, sorted(stats))
