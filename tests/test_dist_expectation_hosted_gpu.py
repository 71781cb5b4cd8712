"""GPU: Pauli-sum expectation values on the sharded state with one process per rank on one GPU
(host-staged transport, tests/dist_expectation_hosted.py): every rank lowers the terms for its own
shard, posts its own half-shard and adds the totals in rank order.  All ranks must report the same
double, bit for bit; the values must match numpy on the oracle's state at 1e-12 * sum |c|
(apply_pauli / expectation_np / bound copied from tests/test_expectation_gpu.py); perm() must be
left as it was.
"""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def apply_pauli(psi, x, z):
    """P|psi> for the string with masks (x, z): P|i> = i^nY (-1)^popcount(i & z) |i ^ x>."""
    idx = np.arange(psi.size, dtype=np.uint64)
    par = np.zeros(psi.size, dtype=np.int64)
    t = idx & np.uint64(z)
    while t.any():
        par ^= (t & np.uint64(1)).astype(np.int64)
        t >>= np.uint64(1)
    ny = bin(x & z).count("1")
    out = np.empty_like(psi)
    out[(idx ^ np.uint64(x)).astype(np.int64)] = (1j ** ny) * (1 - 2 * par) * psi
    return out


def expectation_np(psi, terms):
    return sum(c * np.vdot(psi, apply_pauli(psi, x, z)).real for x, z, c in terms)


def bound(terms):
    return 1e-12 * sum(abs(c) for _, _, c in terms)


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
def test_rank_processes_agree_on_expectation_values(qsim, oracle, tmp_path, world, n):
    sys.path.insert(0, HERE)
    import dist_expectation_hosted as helper
    ports = _ports(world)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    procs = [subprocess.Popen([sys.executable, "-u", os.path.join(HERE, "dist_expectation_hosted.py"), str(r),
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
        for key in ("singles", "mixed", "mixed_again"):        # hex floats: the identical double
            assert rec[key] == recs[0][key], (key, rec["rank"])
        assert rec["mixed_again"] == rec["mixed"]
        assert abs(rec["total"] - 1.0) < 1e-12
    g = oracle.gates_of(helper.circuit(qsim, n))
    ref = oracle.run_cpu(n, g + g)
    singles, mixed = helper.cases(n, world, perm)
    L = n - (world.bit_length() - 1)
    phys_x = [sum(1 << perm[q] for q in range(n) if x >> q & 1) for x, _ in singles]
    assert sum(1 for x in phys_x if x >> L) >= 7 and any(x and not x >> L for x in phys_x)
    assert len(mixed) == 60
    for (x, z), v in zip(singles, recs[0]["singles"]):
        assert abs(float.fromhex(v) - expectation_np(ref, [(x, z, 1.0)])) < 1e-12, (hex(x), hex(z))
    assert abs(float.fromhex(recs[0]["mixed"]) - expectation_np(ref, mixed)) <= bound(mixed)
