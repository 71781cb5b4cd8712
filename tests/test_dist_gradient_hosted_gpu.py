"""GPU: adjoint gradients on the sharded state with one process per rank on one GPU (host-staged
transport, tests/dist_gradient_hosted.py): every rank plans the sweep for its own shard, posts its
own whole-shard transfers and joins one vector all-reduce.  All ranks must report the same doubles,
bit for bit; value and gradient must match numpy (tests/gradient_cases.py) on the oracle's state at
gc.bound(terms) = 1e-12 * sum |c|; perm() must end where a run-only twin's ends.
"""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import gradient_cases as gc

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
def test_rank_processes_agree_on_gradients(qsim, oracle, tmp_path, world, n):
    sys.path.insert(0, HERE)
    import dist_gradient_hosted as helper
    from qsim_amd.dist import gradient_plan
    ports = _ports(world)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    procs = [subprocess.Popen([sys.executable, "-u", os.path.join(HERE, "dist_gradient_hosted.py"), str(r),
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
    gates, terms = helper.case(world, n)
    info = gradient_plan(gc.to_circuit(qsim, n, gates), world, terms, perm)
    assert info["steps_cross"] + info["steps_cross_crank"] >= 1 and info["steps_diag"] >= 1, info
    assert info["steps_local_crank"] >= 1 and info["apply_transfers"] >= 1 and info["remap_segments"] >= 1, info
    for rec in recs:
        assert rec["perm_before"] == perm, rec["rank"]
        assert rec["perm_after"] == rec["twin_perm_after"] == info["perm_after_run"], rec["rank"]
        for key in ("value", "grad", "value2", "grad2"):       # hex floats: the identical doubles
            assert rec[key] == recs[0][key], (key, rec["rank"])
        assert abs(rec["total"] - 1.0) < 1e-12
    g0 = oracle.gates_of(helper.circuit(qsim, n))
    psi0 = oracle.run_cpu(n, g0 + g0)
    bar = gc.bound(terms)
    for vk, gk in (("value", "grad"), ("value2", "grad2")):
        wv, wg = gc.adjoint_gradient(psi0, n, gates, terms)
        v = float.fromhex(recs[0][vk])
        g = np.array([float.fromhex(x) for x in recs[0][gk]])
        print(f"{vk}: |dE| = {abs(v - wv):.3e}, max |dgrad| = {np.max(np.abs(g - wg)):.3e}, bar = {bar:.3e}")
        assert abs(v - wv) <= bar and np.max(np.abs(g - wg)) <= bar
        psi0 = gc.run(psi0, n, gates)                          # the second call starts where the first ended
