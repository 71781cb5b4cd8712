"""The oracle of the batched physical-noise process (oracle/numpy_oracle.py:
batched_physical_draws, batched_physical_run), checked without a GPU: against run_cpu where no
hash is involved (p = 1 channels), the order of a step's picks, the draw law's rates and its
independence over (step, channel, trajectory), the damping entries' filtered indexing, and that
every case of tests/test_batched_physical_gpu.py really draws X, Y and Z picks around gates the
engine has to conjugate by its Pauli frame."""
import math

import numpy as np
import pytest

import batched_physical_cases as bc

TOL = 1e-12


def test_p1_channels_equal_explicit_pauli_gates(oracle):
    n, B = 4, 3
    gates = bc.mixed_gates(n, 25, 5)
    channels = [(bc.BIT_FLIP, 0, 1.0), (bc.PHASE_FLIP, 2, 1.0), (bc.BIT_PHASE_FLIP, 3, 1.0),
                (bc.PHASE_FLIP, 0, 1.0)]
    explicit = []
    for g in gates:
        explicit += [g, (bc.X, [0], 0.0), (bc.Z, [2], 0.0), (bc.Y, [3], 0.0), (bc.Z, [0], 0.0)]
    want = oracle.run_cpu(n, explicit)
    got, step = oracle.batched_physical_run(n, B, gates, channels, seed=123)
    assert step == len(gates)
    for t in range(B):
        np.testing.assert_allclose(got[t], want, atol=TOL, rtol=0)


def test_picks_apply_in_channel_order(oracle):
    """[BitFlip q, PhaseFlip q] at p = 1 is Z X on the state: (a, b) -> (b, -a), not X Z's (-b, a)."""
    th = 0.9
    gates = [(bc.RY, [0], th)]
    a, b = math.cos(th / 2), math.sin(th / 2)
    got, _ = oracle.batched_physical_run(1, 2, gates, [(bc.BIT_FLIP, 0, 1.0), (bc.PHASE_FLIP, 0, 1.0)], seed=1)
    for t in range(2):
        np.testing.assert_allclose(got[t], [b, -a], atol=TOL, rtol=0)
    got, _ = oracle.batched_physical_run(1, 2, gates, [(bc.PHASE_FLIP, 0, 1.0), (bc.BIT_FLIP, 0, 1.0)], seed=1)
    for t in range(2):
        np.testing.assert_allclose(got[t], [-b, a], atol=TOL, rtol=0)


def test_draw_law_rates(oracle):
    """One Depolarizing entry over 2^16 (step, trajectory) draws: fire rate p, each Pauli p / 3,
    within 6 binomial standard errors."""
    p, steps, trajs = 0.3, 256, 256
    draws = steps * trajs
    assert draws == 1 << 16
    count = [0, 0, 0]
    for s in range(steps):
        for t in range(trajs):
            for pauli, q in oracle.batched_physical_draws([(bc.DEPOLARIZING, 2, p)], 2024, s, t):
                assert q == 2
                count[pauli] += 1
    se = lambda r: math.sqrt(r * (1.0 - r) / draws)
    assert abs(sum(count) / draws - p) < 6 * se(p)
    for k in range(3):
        assert abs(count[k] / draws - p / 3) < 6 * se(p / 3)


def test_draws_differ_over_step_channel_and_trajectory(oracle):
    p = 0.5
    channels = [(bc.BIT_FLIP, 0, p), (bc.BIT_FLIP, 1, p), (bc.BIT_FLIP, 2, p)]
    steps, trajs = 24, 24
    fired = np.zeros((steps, len(channels), trajs), bool)
    for s in range(steps):
        for t in range(trajs):
            for _, q in oracle.batched_physical_draws(channels, 7, s, t):
                fired[s, q, t] = True
    # the uniforms themselves: the key of every (step, channel, trajectory) triple is its own
    keys = {oracle._mix(7 ^ oracle._mix(s * 0x100000001b3 + c) ^ (t << 20))
            for s in range(steps) for c in range(len(channels)) for t in range(trajs)}
    assert len(keys) == steps * len(channels) * trajs
    for c in range(len(channels)):
        for d in range(c + 1, len(channels)):
            assert not np.array_equal(fired[:, c, :], fired[:, d, :])  # two channels of equal p
    for t in range(trajs):
        for u in range(t + 1, trajs):
            assert not np.array_equal(fired[:, :, t], fired[:, :, u])  # two trajectories
    for s in range(steps):
        for r in range(s + 1, steps):
            assert not np.array_equal(fired[s], fired[r])  # two steps
    assert 0.4 < fired.mean() < 0.6


def test_damping_entries_only_shift_the_model_index(oracle):
    n, B = 3, 4
    gates = bc.mixed_gates(n, 15, 9)
    with_damping = bc.mixed_channels(n, 9)
    without = [c for c in with_damping if c[0] not in (bc.AMPLITUDE_DAMPING, bc.PHASE_DAMPING)]
    assert len(without) == len(with_damping) - 2
    for s in range(10):
        for t in range(B):
            assert oracle.batched_physical_draws(with_damping, 5, s, t) == \
                oracle.batched_physical_draws(without, 5, s, t)
    a, sa = oracle.batched_physical_run(n, B, gates, with_damping, seed=5)
    b, sb = oracle.batched_physical_run(n, B, gates, without, seed=5)
    np.testing.assert_array_equal(a, b)
    assert sa == sb == len(gates)
    # a model of damping entries only draws nothing and leaves the step counter alone
    c, sc = oracle.batched_physical_run(n, B, gates, [(bc.AMPLITUDE_DAMPING, 0, 0.3)], seed=5, step=4)
    assert sc == 4
    for t in range(B):
        np.testing.assert_allclose(c[t], oracle.run_cpu(n, gates), atol=TOL, rtol=0)


def test_step_and_trajectory_offsets_continue_the_stream(oracle):
    """A run split in two (step handed on) and an ensemble split in two (trajectory offset) hold
    the trajectories of the whole; gates the reference gate set skips still draw."""
    n, B = 3, 6
    gates, channels = bc.mixed_gates(n, 16, 3), bc.mixed_channels(n, 3)
    whole, step = oracle.batched_physical_run(n, B, gates, channels, seed=11)
    half, s1 = oracle.batched_physical_run(n, B, gates[:7], channels, seed=11)
    both, s2 = oracle.batched_physical_run(n, B, gates[7:], channels, seed=11, step=s1, states=half)
    assert (s1, s2, step) == (7, 16, 16)
    np.testing.assert_array_equal(both, whole)
    upper, _ = oracle.batched_physical_run(n, 2, gates, channels, seed=11, traj0=4)
    np.testing.assert_array_equal(upper, whole[4:])
    ref, sr = oracle.batched_physical_run(n, B, gates, channels, seed=11, reference_gateset=True)
    assert sr == 16 and any(g[0] not in (0, 1, 2, 3, 11) for g in gates)
    assert np.max(np.abs(ref - whole)) > 1e-3


def _assert_live(oracle, runs, B, traj0, n):
    """runs: [(gates, channels, seed, first step)] in order.  The draws hold an X, a Y and a Z
    pick, at least one pick lands on a step whose gate is not Clifford, and at least one precedes
    a later non-Clifford gate on its own qubit (so a frame it is part of gets conjugated)."""
    seen, on_non_clifford, before_non_clifford = set(), 0, 0
    for gates, channels, seed, step0 in runs:
        if not channels:
            continue
        for i, g in enumerate(gates):
            for b in range(B):
                for pauli, q in oracle.batched_physical_draws(channels, seed, step0 + i, traj0 + b):
                    assert 0 <= q < n
                    seen.add(pauli)
                    on_non_clifford += g[0] not in bc.CLIFFORD
                    before_non_clifford += any(h[0] not in bc.CLIFFORD and q in h[1] for h in gates[i + 1:])
    assert seen == {0, 1, 2}
    assert on_non_clifford > 0 and before_non_clifford > 0


@pytest.mark.parametrize("name", list(bc.RANDOM_CASES))
def test_random_cases_draw_every_pauli_around_non_clifford_gates(oracle, name):
    case = bc.RANDOM_CASES[name]
    _assert_live(oracle, bc.case_runs(case), case["B"], case["traj0"], case["n"])
    types = {c[0] for c in bc.mixed_channels(case["n"], case["cseed"])}
    assert types == set(range(6))
    assert all(0.1 <= c[2] <= 0.5 for c in bc.mixed_channels(case["n"], case["cseed"]))


@pytest.mark.parametrize("name", bc.SCENARIOS)
def test_scenarios_draw_every_pauli_around_non_clifford_gates(oracle, name):
    sc = bc.scenario(name)
    step, runs = 0, []
    for gates, channels, how in sc["stages"]:
        if how == "sync":
            continue
        runs.append((gates, channels, sc["seed"], step))
        step += len(gates) if channels else 0
    # every noisy run on its own already qualifies (the first one is what a reader meets)
    for r in runs:
        if r[1]:
            _assert_live(oracle, [r], sc["B"], 0, sc["n"])


def test_frame_matrix_covers_what_it_claims():
    """Every role of every gate sees a lowest, a middle and the top qubit; one- and two-qubit
    gates all 4^k frames at n = 10, Toffoli all 64 at one placement; everywhere else every
    operand sits under each of I, X, Y, Z."""
    for n, size in bc.FRAME_SIZES.items():
        lo, hi = min(size["operands"]), max(size["operands"])
        assert lo == 0 and hi == n - 1
        for gt in range(17):
            cases = bc.frame_cases(n, gt)
            k = bc.ARITY[gt]
            by_place = {}
            for ops, fr, fillers in cases:
                assert set(ops) <= set(size["operands"]) and size["spare"] not in ops
                assert len(set(ops)) == k == len(fr)
                by_place.setdefault(ops, set()).add((fr, fillers))
            for role in range(k):
                seen = {ops[role] for ops in by_place}
                assert lo in seen and hi in seen and any(lo < q < hi for q in seen)
            for i, (ops, frs) in enumerate(by_place.items()):
                assert {f for _, f in frs} == {1, 2}
                strings = {s for s, _ in frs}
                for role in range(k):
                    assert {s[role] for s in strings} == set("IXYZ")
                if n == 10 and (k < 3 or i == 0):
                    assert len(strings) == 4 ** k
