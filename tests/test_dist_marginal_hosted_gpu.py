"""GPU: marginal probabilities and reduced density matrices on the sharded state with one process
per rank on one GPU (host-staged transport, tests/dist_marginal_hosted.py): every rank lowers the
qubits for its own shard, posts its own (half) shard and the vectors are added in rank order.  All
ranks must report the same doubles, bit for bit, a repeated call too; the values must match numpy
on the oracle's state at marginal_cases.ATOL; perm() must be left as it was.
"""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import marginal_cases as mc

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


def _floats(hexes):
    return np.array([float.fromhex(h) for h in hexes])


@pytest.mark.subprocess  # started before this process initialises the GPU (pool rule)
@pytest.mark.parametrize("world,n", [(4, 10), (8, 10)])
def test_rank_processes_agree_on_marginals_and_matrices(qsim, oracle, tmp_path, world, n):
    sys.path.insert(0, HERE)
    import dist_marginal_hosted as helper
    ports = _ports(world)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    procs = [subprocess.Popen([sys.executable, "-u", os.path.join(HERE, "dist_marginal_hosted.py"), str(r),
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
    for rec in recs:
        assert rec["perm_before"] == perm and rec["perm_after"] == perm, rec["rank"]
        for key in ("marginals", "matrices"):                  # hex floats: the identical doubles
            assert rec[key] == recs[0][key], (key, rec["rank"])
            assert rec[key + "_again"] == rec[key], (key, rec["rank"])
        assert abs(rec["total"] - 1.0) < 1e-12
    g = oracle.gates_of(helper.circuit(qsim, n))
    ref = oracle.run_cpu(n, g + g)
    marg, rdm = helper.cases(n, world, perm)
    L = n - (world.bit_length() - 1)
    on_rank = lambda qs: sum(1 for q in qs if perm[q] >= L)
    assert any(on_rank(qs) == n - L for qs in marg) and any(on_rank(qs) == n - L for qs in rdm)
    assert any(0 < on_rank(qs) < len(qs) for qs in rdm) and any(qs and on_rank(qs) == 0 for qs in rdm)
    for qs, v in zip(marg, recs[0]["marginals"]):
        assert np.max(np.abs(_floats(v) - mc.marginal_np(ref, qs))) <= mc.ATOL, qs
    for qs, v in zip(rdm, recs[0]["matrices"]):
        rho = _floats(v).view(np.complex128).reshape(1 << len(qs), 1 << len(qs))
        assert np.max(np.abs(rho - mc.rdm_np(ref, qs))) <= mc.ATOL, qs
        assert np.array_equal(rho, rho.conj().T), qs
