"""Test helper: one rank process of a multi-process sharded EXPECTATION-VALUE run without RCCL
(the host-staged transport over tests/dist_hosted.py's SocketMesh).

Run as a script: python dist_expectation_hosted.py RANK WORLD PORTS N OUT_DIR
Every rank runs one circuit twice, then evaluates the single strings and the mixed sum of
`cases(n, world, perm)` — chosen by physical position through the rank's own perm(), which is the
same on every rank — and writes the values (as hex floats: compared bit for bit) with perm()
before and after to OUT_DIR/rank<R>.json.
"""
from __future__ import annotations

import json
import os
import sys


def circuit(q, n):
    return q.createRandomHCCircuit(n, 100, 42)


def _mask(positions):
    m = 0
    for p in positions:
        m |= 1 << p
    return m


def _to_logical(perm, m):
    return sum(1 << q for q in range(len(perm)) if m >> perm[q] & 1)


def cases(n, world, perm):
    """(single strings [(x, z)], mixed sum [(x, z, c)]) in LOGICAL masks."""
    import numpy as np
    g = world.bit_length() - 1
    L = n - g
    b = L - 1
    ranks = list(range(L, n))
    phys = [(_mask([L]), 0), (_mask([L, 1]), _mask([L, 0])), (_mask([n - 1, b]), _mask([b, 3])),
            (_mask([n - 1, b, 2]), _mask([n - 1, b, 2, L])), (_mask(ranks), _mask([0])),
            (_mask(ranks + [b, 6]), _mask(ranks[:1] + [6])), (_mask(ranks + [1, 3]), _mask([ranks[-1], 1, 3, 0])),
            (_mask([1]), _mask([n - 1])), (_mask([b, 2]), _mask([2, L])), (0, _mask([0, L, n - 1])), (0, 0)]
    singles = [(_to_logical(perm, x), _to_logical(perm, z)) for x, z in phys]
    rng = np.random.default_rng(17)
    xs = [0, _mask([1]), _mask([b, 2]), _mask([L]), _mask([L, 1]), _mask([L, 0, 3]), _mask([L, b]),
          _mask([n - 1, b, 2]), _mask(ranks + [1])]
    counts = [3, 3, 3, 3, 40, 2, 2, 2, 2]
    mixed = []
    for x, k in zip(xs, counts):
        zs = sorted({int(v) for v in rng.choice(1 << n, size=k, replace=False)})
        mixed += [(_to_logical(perm, x), _to_logical(perm, z), float(rng.uniform(-1, 1))) for z in zs]
    return singles, mixed


def pauli_sum(q, n, terms):
    h = q.PauliSum(n)
    for x, z, c in terms:
        f = {}
        for b in range(n):
            xb, zb = x >> b & 1, z >> b & 1
            if xb or zb:
                f[b] = "Y" if xb and zb else ("X" if xb else "Z")
        h.add(c, f)
    return h


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
    singles, mixed = cases(n, world, perm)
    rec = {"rank": rank, "perm_before": perm}
    rec["singles"] = [d.expectation(pauli_sum(q, n, [(x, z, 1.0)])).hex() for x, z in singles]
    h = pauli_sum(q, n, mixed)
    rec["mixed"] = d.expectation(h).hex()
    rec["mixed_again"] = d.expectation(h).hex()
    rec["perm_after"] = d.perm()
    rec["total"] = d.getTotalProbability()
    d.close()
    mesh.close()
    with open(os.path.join(out, f"rank{rank}.json"), "w") as f:
        json.dump(rec, f)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
