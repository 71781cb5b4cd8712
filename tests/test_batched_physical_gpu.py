"""BatchedSimulator(noise=Physical) against an oracle written outside the engine
(oracle/numpy_oracle.py: batched_physical_run — every gate through run_cpu, then every drawn
Pauli as its textbook matrix; no composed Pauli strings, no frames, no Clifford rules).

Every trajectory's full complex amplitudes at 1e-12 per component (the project's bar; applying a
Pauli is exact), so a wrong pick, a wrong phase of a composed step, a repeated uniform or a wrong
sign in a frame rule fails here even where the fused and the per-gate execution agree with each
other (tests/test_batched_gpu.py).  The cases are tests/batched_physical_cases.py's;
tests/test_batched_physical_cpu.py checks on the CPU that each of them draws X, Y and Z picks
around non-Clifford gates.
  a. random draws: per-gate launch shapes (n < 10, odd B), fused frames (n >= 10), consecutive
     runs, reseeding, a trajectory offset, the reference gate set, carried frames through mixed
     runs, relabeled trajectories, specialised kernels;
  b. a deterministic matrix (p = 1 channels): every gate type under every Pauli on every operand;
  c. every reader of a state whose frame is still pending."""
import functools

import numpy as np
import pytest

import batched_physical_cases as bc

pytestmark = pytest.mark.gpu
TOL = 1e-12


def _assert_states(sim, want):
    for t in range(want.shape[0]):
        np.testing.assert_allclose(sim.getStateVector(t), want[t], atol=TOL, rtol=0,
                                   err_msg=f"trajectory {t}")


# ---- a. random draws --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random_case_states(name):
    """Oracle states after the first and after the second run of a case (computed once, shared by
    the fused and the per-gate test)."""
    import numpy_oracle as oracle
    case = bc.RANDOM_CASES[name]
    out, st = [], None
    for gates, channels, seed, step0 in bc.case_runs(case):
        st, _ = oracle.batched_physical_run(case["n"], case["B"], gates, channels, seed, step=step0,
                                            traj0=case["traj0"], reference_gateset=case["refset"], states=st)
        st.setflags(write=False)
        out.append(st)
    return out


@pytest.mark.parametrize("per_gate", [False, True], ids=["asked_fused", "per_gate"])
@pytest.mark.parametrize("name", list(bc.RANDOM_CASES))
def test_random_draws_match_oracle(qsim, gpu_ready, name, per_gate):
    case = bc.RANDOM_CASES[name]
    n, B = case["n"], case["B"]
    runs = bc.case_runs(case)
    c = bc.circuit_of(qsim, n, runs[0][0])
    gate_set = qsim.BatchedGateSet.Reference if case["refset"] else qsim.BatchedGateSet.Full
    sim = qsim.BatchedSimulator(n, B, bc.model_of(qsim, runs[0][1]), gate_set=gate_set,
                                noise=qsim.BatchedNoise.Physical)
    sim.setSeed(case["seed"])
    if case["traj0"]:
        sim.setTrajectoryOffset(case["traj0"])
    want = _random_case_states(name)
    sim.run(c, per_gate=per_gate)
    if name in ("n6_B9", "n12_B4"):  # (elsewhere the second run composes the pending frame)
        _assert_states(sim, want[0])
    if case["seed2"] is not None:
        sim.setSeed(case["seed2"])
    sim.run(c, per_gate=per_gate)
    _assert_states(sim, want[1])
    sim.close()


def _run_scenario(qsim, oracle, name, after_first_run=None):
    """Play a scenario's stages on the engine; after EVERY stage compare a twin brought to the
    same point with the oracle (reading materialises the frame, so the object under test is only
    read at the end)."""
    sc = bc.scenario(name)
    n, B = sc["n"], sc["B"]

    def play(upto):
        sim = qsim.BatchedSimulator(n, B, noise=qsim.BatchedNoise.Physical)
        sim.setSeed(sc["seed"])
        for k, (gates, channels, how) in enumerate(sc["stages"][:upto]):
            if how == "sync":
                sim.synchronize()
                continue
            sim.setNoiseModel(bc.model_of(qsim, channels))
            sim.run(bc.circuit_of(qsim, n, gates), per_gate=(how == "per_gate"))
            if k == 0 and after_first_run:
                after_first_run(sim)
        return sim

    st, step = None, 0
    for k, (gates, channels, how) in enumerate(sc["stages"]):
        if how != "sync":
            st, step = oracle.batched_physical_run(n, B, gates, channels, sc["seed"], step=step, states=st)
        sim = play(k + 1)
        _assert_states(sim, st)
        sim.close()


def test_carried_frames_match_oracle_at_every_stage(qsim, oracle, gpu_ready):
    """noisy fused run, noise-free fused run under the carried frame, per-gate run (materialises
    first), noisy fused run, sync, noisy fused run: the oracle's trajectories after every stage."""
    _run_scenario(qsim, oracle, "carried")


def test_relabeled_trajectories_match_oracle(qsim, oracle, gpu_ready):
    """The first fused run from |0..0> relabels the qubits inside every trajectory (threshold
    lowered): channel qubits follow the labels, draws stay keyed by the channel index."""
    from qsim_amd.plan import set_relabel
    n = bc.scenario("relabel")["n"]
    seen = []
    set_relabel(1, 14)
    try:
        _run_scenario(qsim, oracle, "relabel", after_first_run=lambda sim: seen.append(sim.perm()))
    finally:
        set_relabel(1, 26)
    assert seen and all(p != list(range(n)) for p in seen), "expected the planner to relabel this circuit"


def test_specialised_and_interpreted_passes_match_oracle(qsim, oracle, gpu_ready):
    """Kernels compiled inline: the Clifford-only first pass runs as a specialised kernel (the
    frame moves through it), the passes with frame-conjugated gates in the interpreter."""
    from qsim_amd.plan import set_jit
    info = []
    set_jit(2, 0)
    try:
        _run_scenario(qsim, oracle, "jit", after_first_run=lambda sim: info.append(sim.lastRunInfo()))
    finally:
        set_jit(1, 20)
    # (compiled kernels exist; a pass with frame-conjugated gates never launches its own)
    assert info and all(passes >= 2 and jit_passes >= 1 for passes, jit_passes in info), info


# ---- b. deterministic frame matrix ------------------------------------------------------------
@pytest.fixture(scope="module")
def frame_sims(qsim, gpu_ready):
    """One simulator and one prepared oracle state per size, reused through reset()."""
    import numpy_oracle as oracle
    sims = {}
    for n in bc.FRAME_SIZES:
        prep = oracle.run_cpu(n, bc.prep_gates(n))
        prep.setflags(write=False)
        assert np.min(np.abs(prep)) > 1e-6  # every amplitude takes part
        sims[n] = (qsim.BatchedSimulator(n, 3, noise=qsim.BatchedNoise.Physical), prep,
                   bc.circuit_of(qsim, n, bc.prep_gates(n)))
    yield sims
    for sim, _, _ in sims.values():
        sim.close()


@pytest.mark.parametrize("per_gate", [False, True], ids=["fused", "per_gate"])
@pytest.mark.parametrize("gate_type", range(17), ids=bc.NAMES)
def test_frame_matrix(qsim, oracle, frame_sims, gate_type, per_gate):
    """[f x H on a spare qubit, G, T on G's target] with p = 1 Pauli channels on G's operands: G
    meets the frame P (f = 1) or P^2 (f = 2: the identity, through the phase arithmetic), the
    trailing T consumes the frame a Clifford G produced.  Expected: run_cpu with the Paulis as
    explicit gates after every step.  All three trajectories must equal it."""
    quiet = qsim.NoiseModel()
    for n, (sim, prep, prep_circuit) in frame_sims.items():
        for operands, frame, fillers in bc.frame_cases(n, gate_type):
            sim.reset()
            sim.setNoiseModel(quiet)
            sim.run(prep_circuit)
            sim.setNoiseModel(bc.model_of(qsim, bc.frame_channels(operands, frame)))
            sim.run(bc.circuit_of(qsim, n, bc.frame_circuit(n, gate_type, operands, fillers)), per_gate=per_gate)
            want = oracle.run_cpu(n, bc.frame_expected_gates(n, gate_type, operands, frame, fillers), prep)
            for t in range(3):
                np.testing.assert_allclose(
                    sim.getStateVector(t), want, atol=TOL, rtol=0,
                    err_msg=f"n={n} {bc.NAMES[gate_type]}{operands} frame {frame} fillers {fillers} trajectory {t}")


# ---- c. readers under a pending frame ---------------------------------------------------------
@pytest.fixture(scope="module")
def pending(qsim, gpu_ready):
    """(factory of simulators right after one fused noisy run — frame pending —, oracle states)."""
    import numpy_oracle as oracle
    sc = bc.scenario("readers")
    gates, channels, _ = sc["stages"][0]
    want, _ = oracle.batched_physical_run(sc["n"], sc["B"], gates, channels, sc["seed"])
    want.setflags(write=False)
    # the noise moved every trajectory's distribution (else the readers would prove nothing)
    ideal = np.abs(oracle.run_cpu(sc["n"], gates)) ** 2
    assert all(np.max(np.abs(np.abs(want[t]) ** 2 - ideal)) > 1e-3 for t in range(sc["B"]))
    circuit, model = bc.circuit_of(qsim, sc["n"], gates), bc.model_of(qsim, channels)

    def fresh():
        sim = qsim.BatchedSimulator(sc["n"], sc["B"], model, noise=qsim.BatchedNoise.Physical)
        sim.setSeed(sc["seed"])
        sim.run(circuit)
        return sim

    return fresh, want, sc["n"], sc["B"]


def test_trajectory_probabilities_under_pending_frame(pending):
    fresh, want, n, B = pending
    for t in (B - 1, 0, 1, 2):
        sim = fresh()
        np.testing.assert_allclose(sim.getProbabilities(t), np.abs(want[t]) ** 2, atol=TOL, rtol=0)
        sim.close()


def test_average_probabilities_under_pending_frame(pending):
    fresh, want, n, B = pending
    sim = fresh()
    np.testing.assert_allclose(sim.getAverageProbabilities(), (np.abs(want) ** 2).mean(axis=0), atol=TOL, rtol=0)
    sim.close()


def test_expectations_under_pending_frame(qsim, oracle, pending):
    fresh, want, n, B = pending
    terms = [(0.5, {0: "X"}), (-0.3, {n - 1: "Y"}), (0.25, {4: "Z"}), (0.2, {0: "X", 5: "Y", 9: "Z"}),
             (-0.15, {1: "Y", 2: "Y"}), (0.1, {3: "Z", 8: "X"}), (0.05, {})]
    obs = qsim.PauliSum(n)
    for c, f in terms:
        obs.add(c, f)
    code = {"X": 0, "Y": 1, "Z": 2}
    exp = np.zeros(B)
    for t in range(B):
        for c, f in terms:
            v = want[t]
            for q, letter in f.items():
                v = oracle.apply_numpy(v, n, (code[letter], [q], 0.0))
            exp[t] += c * np.vdot(want[t], v).real
    sim = fresh()
    np.testing.assert_allclose(sim.getExpectations(obs), exp, atol=TOL, rtol=0)
    sim.close()


def test_sampling_under_pending_frame(pending):
    fresh, want, n, B = pending
    shots = 200
    u = np.random.default_rng(5).random((B, shots))
    exp = np.empty((B, shots), np.int64)
    for t in range(B):
        cdf = np.add.accumulate(np.abs(want[t]) ** 2)  # sequential, as the reference's partial_sum
        k = np.searchsorted(cdf, u[t], side="left")
        # a uniform within 1e-9 of a CDF step could fall either way: move it to the middle of its bin
        lo = np.where(k > 0, cdf[np.maximum(k, 1) - 1], 0.0)
        hi = cdf[np.minimum(k, cdf.size - 1)]
        close = (u[t] - lo <= 1e-9) | (hi - u[t] <= 1e-9)
        u[t] = np.where(close & (hi - lo > 4e-9), 0.5 * (lo + hi), u[t])
        k = np.searchsorted(cdf, u[t], side="left")
        assert np.all(k < cdf.size)
        assert np.min(np.abs(cdf[None, :] - u[t][:, None])) > 1e-9
        exp[t] = k
    sim = fresh()
    np.testing.assert_array_equal(sim.sampleWith(u), exp)
    sim.close()
