"""Test helper: one rank process of a multi-process sharded MARGINAL / REDUCED-DENSITY-MATRIX run
without RCCL (the host-staged transport over tests/dist_hosted.py's SocketMesh).

Run as a script: python dist_marginal_hosted.py RANK WORLD PORTS N OUT_DIR
Every rank runs one circuit twice, then reads the marginals and matrices of `cases(n, world, perm)`
— chosen by physical position through the rank's own perm(), which is the same on every rank — and
writes the values (as hex floats: compared bit for bit) with perm() before and after to
OUT_DIR/rank<R>.json.
"""
from __future__ import annotations

import json
import os
import sys


def circuit(q, n):
    return q.createRandomHCCircuit(n, 100, 42)


def cases(n, world, perm):
    """(marginal qubit lists, matrix qubit lists) in LOGICAL qubits."""
    g = world.bit_length() - 1
    L = n - g
    b = L - 1
    ranks = list(range(L, n))
    inv = {p: q for q, p in enumerate(perm)}
    marg = [ranks, [n - 1, 0, b, 3], [1, 6], [L, 2], list(range(n)), []]
    rdm = [ranks, [3, L], [b, n - 1], [n - 1, 0, L, 4], [0, 1, 2, 4, 5, L], [2, 5], []]
    uniq = lambda ps: list(dict.fromkeys(ps))
    return [[inv[p] for p in uniq(ps)] for ps in marg], [[inv[p] for p in uniq(ps)] for ps in rdm]


def main(argv) -> int:
    rank, world = int(argv[1]), int(argv[2])
    ports = [int(p) for p in argv[3].split(",")]
    n, out = int(argv[4]), argv[5]
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    sys.path.insert(0, os.path.join(os.path.dirname(here), "cuda-quantum-simulator_amd"))
    import qsim_amd as q
    from qsim_amd.dist import DistributedSimulator
    from dist_hosted import SocketMesh
    mesh = SocketMesh(rank, world, ports)
    d = DistributedSimulator.hosted(n, rank, world, mesh)
    c = circuit(q, n)
    d.run(c)
    d.run(c)
    perm = d.perm()
    marg, rdm = cases(n, world, perm)
    hexes = lambda a: [float(v).hex() for v in a.ravel().view("float64")]
    rec = {"rank": rank, "perm_before": perm}
    rec["marginals"] = [hexes(d.marginalProbabilities(qs)) for qs in marg]
    rec["matrices"] = [hexes(d.reducedDensityMatrix(qs)) for qs in rdm]
    rec["marginals_again"] = [hexes(d.marginalProbabilities(qs)) for qs in marg]
    rec["matrices_again"] = [hexes(d.reducedDensityMatrix(qs)) for qs in rdm]
    rec["perm_after"] = d.perm()
    rec["total"] = d.getTotalProbability()
    d.close()
    mesh.close()
    with open(os.path.join(out, f"rank{rank}.json"), "w") as f:
        json.dump(rec, f)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
