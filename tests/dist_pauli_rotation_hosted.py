"""Test helper: one rank process of a multi-process sharded PAULI-ROTATION run without RCCL (the
host-staged transport over tests/dist_hosted.py's SocketMesh).

Run as a script: python dist_pauli_rotation_hosted.py RANK WORLD PORTS N OUT_DIR
Every rank runs `prepare(q, n)` (the W-HC circuit twice, then a layer of random rotation gates: a
dense, generic state under a map off the identity), calls pauliGradient on `case(world, n, perm)`,
then evolve() for one order-2 TFIM Trotter step, and writes the value and gradient (as hex floats:
compared bit for bit) with perm() before and after to OUT_DIR/rank<R>.json; rank 0 also writes the
gathered states after either call to OUT_DIR/state<k>.npy.
"""
from __future__ import annotations

import json
import os
import sys

TIME = 0.4


def prepare(q, n):
    import gradient_cases as gc
    import numpy as np
    hc = q.createRandomHCCircuit(n, 100, 42)
    layer = gc.to_circuit(q, n, gc.random_gates(np.random.default_rng(n), n, 4 * n, types=gc.PARAMETRIC))
    return [hc, hc, layer]


def case(world, n, perm):
    """(sequence, observable): 18 random rotations, every third one on local positions only, behind
    a first rotation with X / Y factors on a rank position (a cross bra-ket-only step); H with a
    string read inside a shard and one read across ranks for certain."""
    import gradient_cases as gc
    import numpy as np
    import pauli_rotation_cases as pc
    L = n - (world.bit_length() - 1)
    inv = {p: k for k, p in enumerate(perm)}
    lx = lambda positions: sum(1 << inv[p] for p in set(positions))
    local = lx(range(L))
    rng = np.random.default_rng(40 + world)
    seq = [(x & local, z, th) if k % 3 == 1 else (x, z, th)
           for k, (x, z, th) in enumerate(pc.random_rotations(rng, n, 18))]
    seq = [(lx([n - 1, 2]), lx([n - 1, L, 0]), 0.9)] + seq
    terms = gc.random_terms(rng, n, 8, 3) + [(0, lx([0, L]), -0.25), (lx([n - 1, 1]), lx([L, 1]), 0.35)]
    return seq, terms


def main(argv) -> int:
    rank, world = int(argv[1]), int(argv[2])
    ports = [int(p) for p in argv[3].split(",")]
    n, out = int(argv[4]), argv[5]
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    sys.path.insert(0, os.path.join(os.path.dirname(here), "cuda-quantum-simulator_amd"))
    import numpy as np
    import qsim_amd as q
    import gradient_cases as gc
    import pauli_rotation_cases as pc
    from qsim_amd.dist import DistributedSimulator
    from dist_hosted import SocketMesh
    mesh = SocketMesh(rank, world, ports)
    d = DistributedSimulator.hosted(n, rank, world, mesh)
    for c in prepare(q, n):
        d.run(c)
    rec = {"rank": rank, "perm_before": d.perm()}
    seq, terms = case(world, n, rec["perm_before"])
    v, g = d.pauliGradient(gc.to_pauli_sum(q, n, seq), gc.to_pauli_sum(q, n, terms))
    rec["value"], rec["grad"] = v.hex(), [float(x).hex() for x in g]
    rec["perm_after"] = d.perm()
    state = d.getStateVector()                 # collective; the amplitudes on rank 0
    if rank == 0:
        np.save(os.path.join(out, "state0.npy"), state)
    d.evolve(gc.to_pauli_sum(q, n, pc.tfim_terms(n)), TIME, 1, 2)
    rec["perm_after_evolve"] = d.perm()
    rec["total"] = d.getTotalProbability()
    state = d.getStateVector()
    if rank == 0:
        np.save(os.path.join(out, "state1.npy"), state)
    d.close()
    mesh.close()
    with open(os.path.join(out, f"rank{rank}.json"), "w") as f:
        json.dump(rec, f)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
