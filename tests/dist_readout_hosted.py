"""Test helper: one rank process of a multi-process sharded READOUT run without RCCL (the
host-staged transport over tests/dist_hosted.py's SocketMesh).

Run as a script: python dist_readout_hosted.py RANK WORLD PORTS N OUT_DIR
Every rank runs one circuit twice, then getProbabilities, sampleWith(uniforms(n)), sample() with
a DIFFERENT seed per rank (the shots must still agree: rank 0 draws, the others receive),
measureBit with a fixed uniform on the bit at the highest (rank) position, and the gathers around
them.  Rank 0 saves the arrays; every rank writes what it saw to OUT_DIR/rank<R>.json.
"""
from __future__ import annotations

import json
import os
import sys

MEASURE_UNIFORM = 0.4


def circuit(q, n):
    return q.createRandomHCCircuit(n, 100, 42)


def uniforms(n):
    import numpy as np
    return np.concatenate([np.random.default_rng(4242 + n).random(4000), [1.5]])


def main(argv) -> int:
    rank, world = int(argv[1]), int(argv[2])
    ports = [int(p) for p in argv[3].split(",")]
    n, out = int(argv[4]), argv[5]
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    sys.path.insert(0, os.path.join(os.path.dirname(here), "cuda-quantum-simulator_amd"))
    import numpy as np
    import qsim_amd as q
    from qsim_amd.dist import DistributedSimulator
    from dist_hosted import SocketMesh
    mesh = SocketMesh(rank, world, ports)
    d = DistributedSimulator.hosted(n, rank, world, mesh)
    c = circuit(q, n)
    d.run(c)
    d.run(c)
    rec = {"rank": rank, "perm_before": d.perm()}
    probs = d.getProbabilities()
    assert (probs is None) == (rank != 0)
    shots = d.sampleWith(uniforms(n))
    rec["shots"] = [int(x) for x in shots]
    rec["perm_after"] = d.perm()
    st = d.getStateVector()
    d.setSeed(100 + rank)
    rec["drawn"] = [int(x) for x in d.sample(32)]
    perm = d.perm()
    bit = max(range(n), key=lambda b: perm[b])
    rec["bit"] = bit
    rec["p0"] = d.probBitZero(bit)
    rec["result"] = d.measureBit(bit, uniform=MEASURE_UNIFORM)
    rec["total"] = d.getTotalProbability()
    rec["again"] = d.measureBit(bit, uniform=0.9)
    after = d.getStateVector()
    if rank == 0:
        np.save(os.path.join(out, "probs.npy"), probs)
        np.save(os.path.join(out, "state.npy"), st)
        np.save(os.path.join(out, "measured.npy"), after)
    d.close()
    mesh.close()
    with open(os.path.join(out, f"rank{rank}.json"), "w") as f:
        json.dump(rec, f)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
