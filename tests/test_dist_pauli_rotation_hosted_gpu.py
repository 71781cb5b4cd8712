"""GPU: Pauli-string rotations and their gradients on the sharded state with one process per rank
on one GPU (host-staged transport, tests/dist_pauli_rotation_hosted.py): every rank lowers the
sequence for its own shard, posts its own whole-shard transfers and joins one vector all-reduce.
All ranks must report the same doubles, bit for bit; value, gradient and the gathered state must
match numpy (tests/pauli_rotation_cases.py) on the oracle's start state at 1e-12 per amplitude
component and gc.bound(terms) = 1e-12 * sum |c|; perm() must not move.
"""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import gradient_cases as gc
import pauli_rotation_cases as pc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _ports(k):
    socks, ports = [], []
    for _ in range(k):
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        socks.append(s)
        ports.append(s.getsockname()[1])
    for s in socks:
        s.close()
    return ports


@pytest.mark.subprocess  # started before this process initialises the GPU (pool rule)
@pytest.mark.parametrize("world,n", [(4, 10), (8, 10)])
def test_rank_processes_agree_on_rotations(qsim, oracle, tmp_path, world, n):
    sys.path.insert(0, HERE)
    import dist_pauli_rotation_hosted as helper
    from qsim_amd.dist import pauli_gradient_plan, pauli_rotation_plan
    ports = _ports(world)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    procs = [subprocess.Popen([sys.executable, "-u", os.path.join(HERE, "dist_pauli_rotation_hosted.py"), str(r),
                               str(world), ",".join(map(str, ports)), str(n), str(tmp_path)], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(world)]
    outs = []
    try:
        for p in procs:
            out, _ = p.communicate(timeout=100)
            outs.append(out.decode(errors="replace")[-3000:])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r} failed:\n{outs[r]}"
    recs = [json.load(open(tmp_path / f"rank{r}.json")) for r in range(world)]
    perm = recs[0]["perm_before"]
    assert perm != list(range(n))                              # the map has left the identity
    seq, terms = helper.case(world, n, perm)
    info = pauli_gradient_plan(n, world, perm, seq, terms)
    assert info["forward_cross_rotations"] >= 1 and info["steps_cross"] >= 2 and info["first_class"] == 2, info
    assert info["steps_phase"] >= 1 and info["steps_local"] >= 1 and info["apply_transfers"] >= 1, info
    trotter = pc.trotter_sequence(pc.tfim_terms(n), helper.TIME, 1, 2)
    tinfo = pauli_rotation_plan(n, world, perm, trotter)
    assert tinfo["cross_rotations"] >= 1 and tinfo["phase_passes"] >= 1, tinfo
    for rec in recs:
        assert rec["perm_before"] == rec["perm_after"] == rec["perm_after_evolve"] == perm, rec["rank"]
        for key in ("value", "grad"):                          # hex floats: the identical doubles
            assert rec[key] == recs[0][key], (key, rec["rank"])
        assert abs(rec["total"] - 1.0) < 1e-12
    psi0 = oracle.run_cpu(n, [g for c in helper.prepare(qsim, n) for g in oracle.gates_of(c)])
    wv, wg = pc.sequence_gradient(psi0, seq, terms)
    assert np.abs(wg).max() > 1e-3
    v = float.fromhex(recs[0]["value"])
    g = np.array([float.fromhex(x) for x in recs[0]["grad"]])
    bar = gc.bound(terms)
    print(f"|dE| = {abs(v - wv):.3e}, max |dgrad| = {np.max(np.abs(g - wg)):.3e}, bar = {bar:.3e}")
    assert abs(v - wv) <= bar and np.max(np.abs(g - wg)) <= bar
    psi1 = pc.run_sequence(psi0, seq)
    e0 = pc.max_component_diff(np.load(tmp_path / "state0.npy"), psi1)
    e1 = pc.max_component_diff(np.load(tmp_path / "state1.npy"), pc.run_sequence(psi1, trotter))
    print(f"state after pauliGradient: {e0:.3e}, after evolve: {e1:.3e}")
    assert e0 < 1e-12 and e1 < 1e-12
