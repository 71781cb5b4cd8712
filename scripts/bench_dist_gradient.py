#!/usr/bin/env python3
"""Timing of adjoint-method gradients on the sharded state (csrc/hip/dist_adjoint.hip) on virtual
ranks of one GPU, with the protocol of scripts/bench_gradient.py.

Circuit: a hardware-efficient ansatz, --layers layers of RY and RZ on every qubit plus a CNOT
ladder (P = 2 x qubits x layers angles).  Observable: a transverse-field Ising chain,
H = -sum Z_q Z_q+1 - 0.7 sum X_q.  After a warm-up of every case, the median, minimum and maximum
of --repeats synchronised calls (host clock; the cases alternate inside every repeat) of

  a  DistributedSimulator.gradient() on --world virtual ranks
  b  Simulator.gradient() on the same circuit (one unsharded state)
  c  one parameter of sharded parameter shift: two shifted run() + two expectation(); c x P is
     what a caller of the sharded simulator had before gradient()
  d  a with QSIM_ADJOINT_FUSED=0 (the local class composed from a reduction and two launches)

and the per-kernel times of one profiled call of (a) from profileStats().  Every case runs on the
state the case before left.  On virtual ranks every transfer is a device copy that competes with
the kernels for the same HBM: nothing about xGMI follows from these figures.  Prints one JSON line.

    python scripts/bench_dist_gradient.py --qubits 28 --world 8 --repeats 10
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-quantum-simulator_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--qubits", type=int, default=28)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--skip-single", action="store_true", help="leave case b out (memory)")
    args = ap.parse_args()
    if args.repeats < 10:
        ap.error("--repeats must be at least 10")

    import numpy as np
    import qsim_amd as q
    from qsim_amd.dist import DistributedSimulator, gradient_plan

    n = args.qubits
    rng = np.random.default_rng(args.seed)
    angles = rng.uniform(-np.pi, np.pi, size=2 * n * args.layers)

    def ansatz(th):
        c = q.Circuit(n)
        a = 0
        for _ in range(args.layers):
            for k in range(n):
                c.ry(k, float(th[a]))
                a += 1
            for k in range(n):
                c.rz(k, float(th[a]))
                a += 1
            for k in range(n - 1):
                c.cnot(k, k + 1)
        return c

    h = q.PauliSum(n)
    for k in range(n - 1):
        h.add(-1.0, {k: "Z", k + 1: "Z"})
    for k in range(n):
        h.add(-0.7, {k: "X"})
    circuit = ansatz(angles)
    P = len(angles)
    d = DistributedSimulator.virtual(n, args.world)
    sim = None if args.skip_single else q.Simulator(n)

    def a_dist():
        os.environ.pop("QSIM_ADJOINT_FUSED", None)  # (read by the engine at every call)
        return d.gradient(circuit, h)

    def b_single():
        return sim.gradient(circuit, h)

    shift_k = [0]

    def c_pair():
        k = shift_k[0] % P
        shift_k[0] += 1
        e = []
        for sign in (1.0, -1.0):
            th = angles.copy()
            th[k] += sign * np.pi / 2
            d.run(ansatz(th))
            e.append(d.expectation(h))
        return (e[0] - e[1]) / 2

    def d_unfused():
        os.environ["QSIM_ADJOINT_FUSED"] = "0"
        try:
            return d.gradient(circuit, h)
        finally:
            os.environ.pop("QSIM_ADJOINT_FUSED", None)

    cases = [("a_dist_gradient", a_dist), ("c_dist_parameter_shift_pair", c_pair), ("d_dist_gradient_unfused", d_unfused)]
    if sim is not None:
        cases.insert(1, ("b_single_gradient", b_single))
    for _ in range(2):  # warm-up, excluded (plans, work shards, first-run layout)
        for _, fn in cases:
            fn()
    times = {name: [] for name, _ in cases}
    for _ in range(args.repeats):
        for name, fn in cases:
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    plan = gradient_plan(circuit, args.world, h, d.perm())
    d.profile(True)
    a_dist()
    stats = d.profileStats()
    d.profile(False)
    out = {"bench": "dist_gradient", "qubits": n, "world": args.world, "virtual": True, "layers": args.layers,
           "parameters": P, "gates": len(circuit.getGates()), "terms": len(h), "repeats": args.repeats,
           "device": q.device_info(0)["name"],
           "plan": {k: v for k, v in plan.items() if not k.startswith("perm_")},
           "profile_one_call": stats}
    for name, _ in cases:
        t = times[name]
        out[name] = {"median_ms": statistics.median(t) * 1e3, "min_ms": min(t) * 1e3, "max_ms": max(t) * 1e3,
                     "spread_max_over_min": max(t) / min(t)}
    a = out["a_dist_gradient"]["median_ms"]
    out["c_parameter_shift_total_ms"] = P * out["c_dist_parameter_shift_pair"]["median_ms"]  # P x the median pair
    out["c_total_over_a"] = out["c_parameter_shift_total_ms"] / a
    out["d_over_a"] = out["d_dist_gradient_unfused"]["median_ms"] / a
    if sim is not None:
        out["a_over_b"] = a / out["b_single_gradient"]["median_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
