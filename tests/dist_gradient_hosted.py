"""Test helper: one rank process of a multi-process sharded GRADIENT run without RCCL (the
host-staged transport over tests/dist_hosted.py's SocketMesh).

Run as a script: python dist_gradient_hosted.py RANK WORLD PORTS N OUT_DIR
Every rank runs one circuit twice, then calls gradient() on `case(world, n)` twice — from the dense
state and again from where the first call left it — and writes the values and gradients (as hex
floats: compared bit for bit) with perm() before and after to OUT_DIR/rank<R>.json, together with
the perm() of a twin that only ran the same circuits.
"""
from __future__ import annotations

import json
import os
import sys

# gc.random_case seeds whose sweep from the dense start has cross steps, diagonal rank-position
# steps, a control on a rank position, a cross apply group and remapping segments (found with
# qsim_amd.dist.gradient_plan; the test asserts it)
SEEDS = {(4, 10): 1, (8, 10): 6}


def circuit(q, n):
    return q.createRandomHCCircuit(n, 100, 42)


def case(world, n):
    import gradient_cases as gc
    return gc.random_case(SEEDS[(world, n)], n)


def main(argv) -> int:
    rank, world = int(argv[1]), int(argv[2])
    ports = [int(p) for p in argv[3].split(",")]
    n, out = int(argv[4]), argv[5]
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    sys.path.insert(0, os.path.join(os.path.dirname(here), "cuda-quantum-simulator_amd"))
    import qsim_amd as q
    import gradient_cases as gc
    from qsim_amd.dist import DistributedSimulator
    from dist_hosted import SocketMesh
    mesh = SocketMesh(rank, world, ports)
    d = DistributedSimulator.hosted(n, rank, world, mesh)
    pre = circuit(q, n)
    d.run(pre)
    d.run(pre)
    gates, terms = case(world, n)
    c, h = gc.to_circuit(q, n, gates), gc.to_pauli_sum(q, n, terms)
    rec = {"rank": rank, "perm_before": d.perm()}
    v, g = d.gradient(c, h)
    rec["value"], rec["grad"] = v.hex(), [float(x).hex() for x in g]
    rec["perm_after"] = d.perm()
    v, g = d.gradient(c, h, fused=False)       # the circuit once more, per gate
    rec["value2"], rec["grad2"] = v.hex(), [float(x).hex() for x in g]
    rec["total"] = d.getTotalProbability()
    d.close()
    twin = DistributedSimulator.hosted(n, rank, world, mesh)
    twin.run(pre)
    twin.run(pre)
    twin.run(c)
    rec["twin_perm_after"] = twin.perm()
    twin.close()
    mesh.close()
    with open(os.path.join(out, f"rank{rank}.json"), "w") as f:
        json.dump(rec, f)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
