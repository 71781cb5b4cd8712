"""CPU: the host-only plan of marginal probabilities and reduced density matrices on a sharded
state (qsim_dist_marginal_plan, qsim_amd.dist.marginal_plan) against an independent Python
computation, its scratch cap and error codes, and a numpy restatement of the pair rule and the
host finish step of the matrix (csrc/hip/dist_marginal.hip) against marginal_cases.rdm_np on a
state split into shards by hand."""
import ctypes

import numpy as np
import pytest

import marginal_cases as mc

MIB = 1 << 20


def _perms(n):
    rot = [(q + 3) % n for q in range(n)]
    rng = np.random.default_rng(n)
    return [None, rot, [int(v) for v in rng.permutation(n)]]


def _expected(n, world, perm, qubits, rdm):
    """The plan's figures from the definitions, without the library."""
    g = world.bit_length() - 1
    L = n - g
    pos = [perm[q] if perm is not None else q for q in qubits]
    loc = sorted(p for p in pos if p < L)
    k_loc, k_rank = len(loc), len(pos) - len(loc)
    steps = (1 << k_rank) - 1 if rdm else 0
    half = (L - 1) not in pos
    out = {"k_loc": k_loc, "k_rank": k_rank, "cross_steps": steps, "transfers": steps,
           "bytes_sent_per_rank": steps * (16 << (L - 1 if half else L)),
           "allreduce_doubles": 2 << (2 * len(pos)) if rdm else 1 << len(pos),
           "pair_rule": 0 if not steps else (1 if half else 2),
           "launches": 3 + 2 * steps}
    return out, L, loc


def test_symbols_exported(qsim):
    from qsim_amd import _lib
    from qsim_amd.dist import DistributedSimulator, marginal_plan
    lib = ctypes.CDLL(_lib.HIP_LIB_PATH)
    for name in ("qsim_dist_marginal_probabilities", "qsim_dist_reduced_density_matrix", "qsim_dist_marginal_plan"):
        assert hasattr(lib, name), name
    assert _lib.hip.qsim_abi_version() == 2  # additive change
    for name in ("marginalProbabilities", "reducedDensityMatrix", "subsystemPurity", "entanglementEntropy"):
        assert callable(getattr(DistributedSimulator, name))
    assert callable(marginal_plan)


@pytest.mark.parametrize("world", [2, 4, 8])
def test_plan_for_every_subset_of_8_qubits(qsim, world):
    from qsim_amd.dist import marginal_plan
    from qsim_amd.plan import marginal_plan as local_plan
    n = 8
    seen_rules = set()
    for perm in _perms(n):
        for qubits in mc.all_subsets(n):
            for rdm in (False, True):
                if rdm and len(qubits) > 6:
                    continue
                got = marginal_plan(n, world, perm, qubits, rdm)
                want, L, loc = _expected(n, world, perm, qubits, rdm)
                for key, v in want.items():
                    assert got[key] == v, (key, perm, qubits, rdm)
                lp = local_plan(L, loc, None, rdm)             # the shard's plan is lower_marginal's at n = L
                for key in ("k_lo", "k_hi", "slices", "work_groups"):
                    assert got[key] == lp[key], (key, perm, qubits, rdm)
                if want["cross_steps"]:                        # panels of min(n_x, 11) bits, at most 1024 groups
                    n_x = L - 1 if want["pair_rule"] == 1 else L
                    assert got["cross_work_groups"] == min(1 << (n_x - min(n_x, 11)), 1024)
                    assert got["scratch_bytes"] == max(lp["scratch_bytes"],
                                                       got["cross_work_groups"] * (16 << (2 * want["k_loc"])))
                else:
                    assert got["cross_work_groups"] == 0 and got["scratch_bytes"] == lp["scratch_bytes"]
                seen_rules.add(got["pair_rule"])
    assert seen_rules == {0, 1, 2}


@pytest.mark.parametrize("n", [30, 33])
def test_scratch_cap(qsim, n):
    from qsim_amd.dist import marginal_plan
    world, L = 8, n - 3
    for rdm, cap in ((False, 20), (True, 6)):
        for k in range(cap + 1):
            picks = [list(range(k)), list(range(n - k, n)), [(7 * j + 1) % n for j in range(k)],
                     list(range(L - k, L)), ([n - 1, n - 2] + list(range(8, 8 + k)))[:k]]
            for qubits in picks:
                assert len(set(qubits)) == k
                for perm in (None, [(q + 7) % n for q in range(n)]):
                    p = marginal_plan(n, world, perm, qubits, rdm)
                    assert p["scratch_bytes"] <= 64 * MIB, (qubits, rdm, p)
                    assert p["cross_steps"] <= 7
                    # at most one whole shard each way per step
                    assert p["bytes_sent_per_rank"] <= p["cross_steps"] * (16 << L)


def test_plan_errors(qsim):
    from qsim_amd import _lib
    from qsim_amd.dist import marginal_plan
    f = _lib.hip.qsim_dist_marginal_plan
    arr = lambda *q: (ctypes.c_int32 * max(1, len(q)))(*q)
    info = (ctypes.c_int32 * 16)()
    bad, oor = _lib.QSIM_ERR_INVALID_ARGUMENT, _lib.QSIM_ERR_OUT_OF_RANGE
    n, world = 24, 8
    for rdm in (0, 1):
        assert f(n, world, None, arr(1, 4, 1), 3, rdm, info) == bad          # duplicate
        assert f(n, world, None, None, 2, rdm, info) == bad                   # null list with k > 0
        assert f(n, world, None, arr(0, 1), 2, rdm, None) == bad              # null out
        assert f(n, world, None, arr(0, n), 2, rdm, info) == oor
        assert f(n, world, None, arr(-1), 1, rdm, info) == oor
        assert f(n, world, arr(*([0] * n)), arr(0), 1, rdm, info) == bad      # no permutation
        assert f(n, 3, None, arr(0), 1, rdm, info) == bad                     # world no power of two
        assert f(n, world, None, None, 0, rdm, info) == _lib.QSIM_OK          # k = 0: the norm
    assert f(n, world, None, arr(*range(21)), 21, 0, info) == bad             # above the caps
    assert f(n, world, None, arr(*range(20)), 20, 0, info) == _lib.QSIM_OK
    assert f(n, world, None, arr(*range(7)), 7, 1, info) == bad
    assert f(n, world, None, arr(*range(18, 24)), 6, 1, info) == _lib.QSIM_OK
    assert f(8, 2, None, arr(*range(8)), 9, 0, info) == bad                   # k above n
    with pytest.raises(ValueError):
        marginal_plan(10, 4, None, [1, 1])
    with pytest.raises(IndexError):
        marginal_plan(10, 4, None, [10])
    with pytest.raises(ValueError):
        marginal_plan(10, 4, [0, 1], [1])


# ---- the pair rule and the finish step, restated on the host -------------------------------------

def _finish(raw, k_loc, dst):
    """dist_rdm_finish: raw is numbered by ascending physical position (local bits, then the
    selected rank bits); dst[i] is the caller's bit of raw bit i."""
    D = raw.shape[0]
    m = np.zeros_like(raw)
    for r in range(D):
        for c in range(D):
            sr, sc = r >> k_loc, c >> k_loc
            if sr == sc:
                m[r, c] = raw[r, c]
            elif sr < sc:
                m[r, c] = raw[r, c] + np.conj(raw[c, r])
    for r in range(D):
        for c in range(D):
            if r >> k_loc > c >> k_loc:
                m[r, c] = np.conj(m[c, r])
    place = lambda t: sum((t >> i & 1) << dst[i] for i in range(len(dst)))
    out = np.zeros_like(raw)
    for r in range(D):
        for c in range(D):
            a, b = place(r), place(c)
            if a > b:
                continue
            v = m[r, c] if a != b else complex(m[r, c].real, 0.0)
            out[a, b] = v
            out[b, a] = np.conj(v)
    return out


def _sharded_rdm(psi, world, perm, qubits):
    """rho of `qubits` from the shards of psi under `perm`, block by block as the engine forms them."""
    n = len(perm)
    g = world.bit_length() - 1
    L = n - g
    idx = np.arange(1 << n)
    phys_of = np.zeros(1 << n, dtype=np.int64)
    for q in range(n):
        phys_of |= ((idx >> q) & 1) << perm[q]
    phys = np.empty_like(psi)
    phys[phys_of] = psi
    shards = phys.reshape(world, 1 << L)
    pos = [perm[q] for q in qubits]
    order = sorted(pos)
    dst = [pos.index(p) for p in order]
    loc = [p for p in order if p < L]
    rank_bits = [p - L for p in order if p >= L]
    k_loc, k = len(loc), len(pos)
    s_of = lambda r: sum((r >> b & 1) << j for j, b in enumerate(rank_bits))
    M = [mc._split(sh, loc) for sh in shards]                   # columns: ascending unselected positions
    half = (L - 1) not in pos
    B = M[0].shape[1]
    raw = np.zeros((1 << k, 1 << k), dtype=np.complex128)
    blk = lambda s, t: (slice(s << k_loc, (s + 1) << k_loc), slice(t << k_loc, (t + 1) << k_loc))
    for r in range(world):
        raw[blk(s_of(r), s_of(r))] += M[r] @ M[r].conj().T
    rank_sel = sum(1 << b for b in rank_bits)
    for d in range(1, world):
        if d & ~rank_sel:
            continue
        for r in range(world):
            peer = r ^ d
            if half:                                           # position L-1 is the columns' top bit
                cols = slice(0, B // 2) if r < peer else slice(B // 2, B)
            elif r < peer:
                cols = slice(0, B)
            else:
                continue
            raw[blk(s_of(r), s_of(peer))] += M[r][:, cols] @ M[peer][:, cols].conj().T
    return _finish(raw, k_loc, dst)


@pytest.mark.parametrize("world", [2, 4, 8])
def test_finish_step_restated_on_a_hand_split_state(world):
    n = 8
    rng = np.random.default_rng(5 + world)
    psi = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
    psi /= np.linalg.norm(psi)
    perm = [int(v) for v in np.random.default_rng(77).permutation(n)]
    L = n - (world.bit_length() - 1)
    inv = [perm.index(p) for p in range(n)]
    cases = [[inv[L]], [inv[n - 1], inv[0]], [inv[L - 1], inv[L]], [inv[2], inv[n - 1], inv[L], inv[0]],
             [inv[p] for p in range(L, n)], [inv[1], inv[3]], [], [inv[n - 1], inv[L - 1], inv[1], inv[L - 2]]]
    for qubits in cases:
        qubits = list(dict.fromkeys(qubits))
        got = _sharded_rdm(psi, world, perm, qubits)
        assert np.max(np.abs(got - mc.rdm_np(psi, qubits))) <= mc.ATOL, qubits
        assert np.array_equal(got, got.conj().T)
