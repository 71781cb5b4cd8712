"""Overlap matrices of a BatchedSimulator ensemble on the device (BatchedSimulator.overlapMatrix,
kernelMatrix, overlapsWith -> qsim_batch_overlaps, qsim_batch_state_overlaps;
csrc/hip/batch_overlap.hip).

Tolerance (derived, not measured): each component of <a|b> sums 2 * 2^n products whose absolute
values sum to at most |a||b|, so any summation order errs by at most 2^(n+1) * 2^-53 * |a||b|, and
so does the numpy value it is compared with: tol(n) = 2 * 2^(n+1) * 2^-53 * |a||b| per component
(1.8e-12 at n = 12 for unit vectors).  That bound is used wherever the device result is compared
with numpy on the states the device itself returns; against the oracle's states and closed forms
(members that come from a run) it is max(tol(n), 1e-12), the project's per-component bound.
Every test handles at most a few MiB of state."""
import numpy as np
import pytest

from test_batch_sweep_gpu import _add, _batch, _oracle_states, _per_gate_circuit, _random_circuit, _slots

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
TOL_RUN = 1e-12


def tol(n, na=1.0, nb=1.0):
    return 2.0 * 2.0 ** (n + 1) * U * na * nb


def _tol_matrix(n, A, B):
    return tol(n, np.linalg.norm(A, axis=1)[:, None], np.linalg.norm(B, axis=1)[None, :])


def _worst(got, want, bound):
    """Largest component error over its bound (< 1 passes) and where."""
    d = got - want
    r = np.maximum(np.abs(d.real), np.abs(d.imag)) / bound
    k = np.unravel_index(int(np.argmax(r)), r.shape)
    return float(r[k]), k


def _assert_close(got, want, bound, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    r, k = _worst(got, want, bound)
    print(f"{what}: worst component error / bound = {r:.3g} at {k}")
    assert r < 1.0, (what, k, r)


def _idle_qubit_circuit(q, seed):
    """13 qubits, a 60-gate random circuit on all of them but qubit 2.  The fused passes work on
    tiles of 12 qubits that always hold the lowest four, so the 12 busy qubits fit one tile only
    under other labels than the identity: with relabeling on from 13 qubits (_relabeling) the
    first fused run from |0..0> leaves perm() != identity.  (At 12 qubits every labeling is one
    tile and the planner keeps the identity.)"""
    live = [k for k in range(13) if k != 2]
    c = q.Circuit(13)
    for g in _random_circuit(q, 12, 60, seed).getGates():
        qs = [live[k] for k in g.qubits] + [0, 0]
        _add(c, int(g.type), qs[0], qs[1], qs[2], float(g.parameter))
    return c


class _relabeling:
    """Layout-aware relabeling of first fused runs from 12 qubits up, inside the block."""

    def __enter__(self):
        from qsim_amd.plan import set_relabel
        set_relabel(1, 12)

    def __exit__(self, *exc):
        from qsim_amd.plan import set_relabel
        set_relabel(1, 26)


def _swept(q, n, B, seed, per_gate=False):
    """B members from |0..0> through one sweep with random angles: every parameterised type; the
    per-gate kernels below 10 qubits (or on request), else a 60-gate random circuit on the fused
    path (n = 13: _idle_qubit_circuit).  Returns (sim, circuit, angles)."""
    c = _per_gate_circuit(q, n) if n < 10 else _idle_qubit_circuit(q, seed) if n == 13 else \
        _random_circuit(q, n, 60, seed)
    a = np.random.default_rng(seed).uniform(-np.pi, np.pi, size=(B, len(_slots(c))))
    sim = _batch(q, n, B)
    sim.runSweep(c, a, per_gate=per_gate)
    return sim, c, a


def _states(sim):
    return np.array([sim.getStateVector(t) for t in range(sim.getBatchSize())])


def _kernels(sim):
    return {s["name"] for s in sim.profileStats() if s["name"].startswith("batch_overlap")}


def _both_paths(sim, monkeypatch, other=None):
    """(matrix-core result, FMA result) of one call each, with the kernels that ran checked."""
    sim.profile(True)
    monkeypatch.setenv("QSIM_OVERLAP_MFMA", "1")
    g1 = sim.overlapMatrix(other)
    ran = _kernels(sim)
    monkeypatch.setenv("QSIM_OVERLAP_MFMA", "0")
    g0 = sim.overlapMatrix(other)
    ran0 = _kernels(sim) - ran
    monkeypatch.delenv("QSIM_OVERLAP_MFMA")
    sim.profile(False)
    cols = g1.shape[1]
    assert ran == {"batch_overlap_mfma" if cols > 1 else "batch_overlap_vec", "batch_overlap_reduce"}, ran
    assert cols == 1 or ran0 == {"batch_overlap_vec"}, ran0
    return g1, g0


# ---- 1. the kernels alone ----
@pytest.mark.parametrize("n", [1, 2, 3, 5, 9])
def test_kernel_alone(qsim, gpu_ready, monkeypatch, n):
    for B in (1, 2, 15, 16, 17, 33, 48):
        sim, _, _ = _swept(qsim, n, B, 100 * n + B)
        g1, g0 = _both_paths(sim, monkeypatch)
        A = _states(sim)
        want, bound = A.conj() @ A.T, _tol_matrix(n, A, A)
        _assert_close(g1, want, bound, f"mfma n={n} B={B}")
        _assert_close(g0, want, bound, f"fma n={n} B={B}")
        _assert_close(g1, g0, bound, f"mfma vs fma n={n} B={B}")


@pytest.mark.parametrize("B", [65, 130])
def test_more_than_one_tile(qsim, gpu_ready, monkeypatch, B):
    """64 members to a tile side: 2 and 3 tiles per side, so tiles off the diagonal (and, at 130,
    one that touches neither the first nor the last row of tiles) and ragged last tiles."""
    from qsim_amd import plan
    n = 5
    info = plan.batch_overlap_plan(n, B)
    assert info["row_tiles"] == (B + 63) // 64 and info["tiles"] == info["row_tiles"] * (info["row_tiles"] + 1) // 2
    sim, _, _ = _swept(qsim, n, B, B)
    g1, g0 = _both_paths(sim, monkeypatch)
    A = _states(sim)
    want, bound = A.conj() @ A.T, _tol_matrix(n, A, A)
    _assert_close(g1, want, bound, f"mfma B={B}")
    _assert_close(g0, want, bound, f"fma B={B}")
    for g in (g1, g0):
        _hermitian_bits(g)


# ---- 2. Hermitian structure ----
def _hermitian_bits(g):
    B = g.shape[0]
    off = ~np.eye(B, dtype=bool)
    assert g.T.conj()[off].tobytes() == g[off].tobytes(), "G[j][i] != conj(G[i][j]) bitwise"
    d = np.ascontiguousarray(np.diagonal(g).imag)
    assert d.tobytes() == np.zeros(B).tobytes(), "diagonal imaginary parts are not +0.0"


@pytest.mark.parametrize("n,B", [(1, 2), (3, 17), (5, 33), (9, 48), (12, 20)])
def test_hermitian_structure(qsim, gpu_ready, monkeypatch, n, B):
    sim, _, _ = _swept(qsim, n, B, 7 * n + B)
    for g in _both_paths(sim, monkeypatch):
        _hermitian_bits(g)
        A = _states(sim)
        norms = (A.real ** 2 + A.imag ** 2).sum(axis=1)
        err = np.abs(np.diagonal(g).real - norms) / tol(n, norms, 1.0)  # (|a||a| = the norm itself)
        assert err.max() < 1.0, (n, B, float(err.max()))


# ---- 3. the fused layout is read where it lies ----
@pytest.mark.parametrize("n", [12, 13])
def test_fused_layout_left_alone(qsim, oracle, gpu_ready, n):
    """A fused sweep, then G against the per-member oracle states; perm() and every member are
    bitwise what they are in a twin that never computed G.  n = 13 (_idle_qubit_circuit): the sweep
    leaves perm() != identity, and G is read under it.  n = 12: this planner keeps the identity at 12
    qubits (one tile whatever the labels), so only the rest is checked there."""
    B = 20
    sim, twin = _batch(qsim, n, B), _batch(qsim, n, B)
    with _relabeling():
        _, c, a = _swept(qsim, n, 1, 77)
        a = np.random.default_rng(78).uniform(-np.pi, np.pi, size=(B, a.shape[1]))
        sim.runSweep(c, a)
        twin.runSweep(c, a)
    before = sim.perm()
    if n == 13:
        assert before != list(range(n)), "expected the planner to relabel this circuit"
    g = sim.overlapMatrix()
    assert sim.perm() == before == twin.perm()
    W = np.array(_oracle_states(oracle, c, a))
    _assert_close(g, W.conj() @ W.T, np.maximum(_tol_matrix(n, W, W), TOL_RUN), "fused layout vs oracle")
    assert sim.perm() == before
    assert _states(sim).tobytes() == _states(twin).tobytes(), "overlapMatrix moved or changed amplitudes"


# ---- 4. more than one K chunk ----
@pytest.mark.parametrize("B", [20, 70])
def test_more_than_one_chunk(qsim, gpu_ready, monkeypatch, B):
    from qsim_amd import plan
    n = 12
    assert plan.batch_overlap_plan(n, B)["chunks"] > 1
    assert plan.batch_overlap_plan(n, B, 1)["chunks"] > 1
    sim, _, _ = _swept(qsim, n, B, 5 + B)
    g1, g0 = _both_paths(sim, monkeypatch)
    A = _states(sim)
    want, bound = A.conj() @ A.T, _tol_matrix(n, A, A)
    _assert_close(g1, want, bound, "mfma, chunked")
    _assert_close(g0, want, bound, "fma, chunked")


# ---- 5. bitwise reproducibility and member independence ----
@pytest.mark.parametrize("n,B,k", [(5, 33, 16), (12, 20, 3)])
def test_reproducible_and_member_independent(qsim, gpu_ready, n, B, k):
    sim, c, a = _swept(qsim, n, B, 41)
    g = sim.overlapMatrix()
    assert sim.overlapMatrix().tobytes() == g.tobytes()
    a2 = a.copy()
    a2[k, :] = np.random.default_rng(42).uniform(-np.pi, np.pi, size=a.shape[1])
    other = _batch(qsim, n, B)
    other.runSweep(c, a2)
    g2 = other.overlapMatrix()
    keep = np.ones((B, B), dtype=bool)
    keep[k, :] = keep[:, k] = False
    assert g2[keep].tobytes() == g[keep].tobytes()
    assert np.abs(g2[k] - g[k]).max() > 1e-3, "member k did not change"


# ---- 6. two ensembles ----
@pytest.mark.parametrize("n", [5, 12, 13])
@pytest.mark.parametrize("Ba,Bb", [(17, 5), (3, 33), (16, 16)])
def test_cross(qsim, gpu_ready, monkeypatch, n, Ba, Bb):
    """n >= 12: a ran a fused sweep, b a per-gate one.  At n = 13 (_idle_qubit_circuit) that leaves
    them in different layouts, which the call has to bring together; at n = 12 this planner keeps
    the identity for both."""
    with _relabeling():
        a, _, _ = _swept(qsim, n, Ba, 11)
        b, _, _ = _swept(qsim, n, Bb, 12, per_gate=True)
    if n == 13:
        assert a.perm() != list(range(n)) and b.perm() == list(range(n))
    g_self = a.overlapMatrix()
    assert a.overlapMatrix(a).tobytes() == g_self.tobytes()
    g1, g0 = _both_paths(a, monkeypatch, b)
    assert g1.shape == (Ba, Bb)
    A, Bm = _states(a), _states(b)
    bound = _tol_matrix(n, A, Bm)
    _assert_close(g1, A.conj() @ Bm.T, bound, f"cross mfma n={n}")
    _assert_close(g0, A.conj() @ Bm.T, bound, f"cross fma n={n}")
    _assert_close(b.overlapMatrix(a), g1.conj().T, bound.T, "the transposed call")
    _assert_close(a.overlapMatrix(), A.conj() @ A.T, _tol_matrix(n, A, A), "self, after the restore")
    _assert_close(g_self, A.conj() @ A.T, _tol_matrix(n, A, A), "self, before the restore")


def test_cross_same_layout_in_place(qsim, gpu_ready):
    """Two ensembles that ran the same fused sweep circuit lie in the same layout, not the
    identity: the cross call reads both where they lie."""
    n = 13
    c = _idle_qubit_circuit(qsim, 77)
    P = len(_slots(c))
    rng = np.random.default_rng(3)
    a, b = _batch(qsim, n, 6), _batch(qsim, n, 9)
    with _relabeling():
        a.runSweep(c, rng.uniform(-3, 3, size=(6, P)))
        b.runSweep(c, rng.uniform(-3, 3, size=(9, P)))
    pa = a.perm()
    assert pa == b.perm() and pa != list(range(n))
    g = a.overlapMatrix(b)
    assert a.perm() == pa and b.perm() == pa, "equal layouts must be read in place"
    A, Bm = _states(a), _states(b)
    _assert_close(g, A.conj() @ Bm.T, _tol_matrix(n, A, Bm), "cross, shared layout")


def test_state_in_another_layout(qsim, gpu_ready):
    """The ensemble lies under perm() != identity, the state under the identity: both are brought to
    one layout first."""
    n, B = 13, 7
    with _relabeling():
        sim, _, _ = _swept(qsim, n, B, 21)
    assert sim.perm() != list(range(n))
    rng = np.random.default_rng(4)
    h = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    got = sim.overlapsWith(h)
    A = _states(sim)
    _assert_close(got[:, None], (A.conj() @ h)[:, None], _tol_matrix(n, A, h[None, :]), "host vector")


# ---- 7. one state against every member ----
@pytest.mark.parametrize("B", [1, 17])
def test_state_overlaps(qsim, gpu_ready, B):
    n = 12
    c = _random_circuit(qsim, n, 60, 5)
    shared = np.array([float(c.getGates()[i].parameter) for i in _slots(c)])
    one = qsim.Simulator(n)
    one.run(c)
    sim = _batch(qsim, n, B)
    sim.runSweep(c, shared)
    v = sim.overlapsWith(one)
    assert v.shape == (B,) and v.dtype == np.complex128
    bound = max(tol(n), TOL_RUN)
    assert np.abs(v.real - 1.0).max() < bound and np.abs(v.imag).max() < bound, v
    assert sim.overlapsWith(one.state).tobytes() == v.tobytes()
    rng = np.random.default_rng(B)
    h = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    got = sim.overlapsWith(h)
    A = _states(sim)
    want = np.array([np.vdot(A[t], h) for t in range(B)])
    _assert_close(got[:, None], want[:, None], _tol_matrix(n, A, h[None, :]), "host vector")


@pytest.mark.parametrize("n", [1, 5])
def test_state_overlaps_small(qsim, gpu_ready, n):
    B = 33
    sim, _, _ = _swept(qsim, n, B, 19)
    rng = np.random.default_rng(n)
    h = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    got = sim.overlapsWith(h)
    A = _states(sim)
    _assert_close(got[:, None], (A.conj() @ h)[:, None], _tol_matrix(n, A, h[None, :]), "host vector")


# ---- 8. pending Pauli frames ----
def test_pending_frames(qsim, gpu_ready):
    n, B = 10, 16
    nm = qsim.NoiseModel()
    nm.addDepolarizingAll(n, 0.05)
    sims = [qsim.BatchedSimulator(n, B, nm, noise=qsim.BatchedNoise.Physical) for _ in range(2)]
    c = _random_circuit(qsim, n, 40, 23)
    for s in sims:
        s.setSeed(99)
        s.run(c)  # fused: the frames of the run are carried, not applied
    g = sims[0].overlapMatrix()  # has to apply them itself
    A = _states(sims[1])
    assert np.abs(A - A[0]).max() > 1e-3, "the noise did nothing"
    _assert_close(g, A.conj() @ A.T, _tol_matrix(n, A, A), "after a noisy fused run")
    assert _states(sims[0]).tobytes() == A.tobytes()


def test_kernel_matrix_is_the_purity(qsim, gpu_ready):
    """mean_ij |G_ij|^2 = Tr rho^2 for rho = mean_t |psi_t><psi_t|.  |x|^2 from components within
    tol errs by at most 2 (|re| + |im|) tol + 2 tol^2 < 3 tol for |x| <= 1, and the numpy side's
    own rounding is below tol: 4 tol(n)."""
    n, B = 4, 16
    nm = qsim.NoiseModel()
    nm.addDepolarizingAll(n, 0.05)
    sim = qsim.BatchedSimulator(n, B, nm, noise=qsim.BatchedNoise.Physical)
    sim.setSeed(7)
    for _ in range(3):
        sim.run(_per_gate_circuit(qsim, n))
    k = sim.kernelMatrix()
    assert k.dtype == np.float64 and k.shape == (B, B)
    A = _states(sim)
    rho = (A.T @ A.conj()) / B
    purity = float(np.trace(rho @ rho).real)
    assert purity < 1.0 - 1e-3, "the noise did nothing"
    assert abs(float(k.mean()) - purity) < 4.0 * tol(n), (float(k.mean()), purity)
    g = sim.overlapMatrix()
    assert (g.real ** 2 + g.imag ** 2).tobytes() == k.tobytes()


# ---- 9. errors ----
def test_errors_leave_both_usable(qsim, gpu_ready):
    a, _, _ = _swept(qsim, 5, 4, 1)
    b, _, _ = _swept(qsim, 6, 3, 2)
    ga, gb = a.overlapMatrix(), b.overlapMatrix()
    with pytest.raises(ValueError):
        a.overlapMatrix(b)
    with pytest.raises(ValueError):
        a.overlapsWith(qsim.Simulator(6))
    with pytest.raises(ValueError):
        a.overlapsWith(np.zeros(1 << 6, dtype=np.complex128))
    assert a.overlapMatrix().tobytes() == ga.tobytes() and b.overlapMatrix().tobytes() == gb.tobytes()
    A = _states(a)
    _assert_close(ga, A.conj() @ A.T, _tol_matrix(5, A, A), "after the errors")


def test_profile_reports_one_read_of_each_operand(qsim, gpu_ready):
    n, Ba, Bb = 5, 17, 5
    a, _, _ = _swept(qsim, n, Ba, 1)
    b, _, _ = _swept(qsim, n, Bb, 2)
    a.profile(True)
    a.overlapMatrix()
    a.overlapMatrix(b)
    stats = {s["name"]: s for s in a.profileStats()}
    assert stats["batch_overlap_mfma"]["launches"] == 2 and stats["batch_overlap_reduce"]["launches"] == 2
    assert stats["batch_overlap_mfma"]["alg_bytes"] == (Ba + Ba + Bb) * 16 * (1 << n)
