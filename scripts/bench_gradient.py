#!/usr/bin/env python3
"""Timing of the adjoint-method gradient (csrc/hip/adjoint.hip) against parameter shift.

Circuit: a hardware-efficient ansatz, --layers layers of RY and RZ on every qubit plus a CNOT
ladder (P = 2 x qubits x layers angles).  Observable: a transverse-field Ising chain,
H = -sum Z_q Z_q+1 - 0.7 sum X_q.  After a warm-up of every case, the median, minimum and maximum
of --repeats synchronised calls (host clock around calls that end in a stream synchronise; the
cases alternate inside every repeat) of

  a  one forward run() + synchronize
  b  gradient() with the fused adjoint step
  c  gradient() with QSIM_ADJOINT_FUSED=0        (bra-ket reduction + two per-gate launches)
  d  parameter shift through run() + expectation(): what a caller had before gradient().  One
     parameter costs two shifted runs and two expectation calls; that pair is timed for --repeats
     different parameters and d = P x the median pair (the full 2P runs are not all executed).

Every case runs on the state the case before left (no reset: a steady-state optimiser loop, no
first-run layout decision inside the timings).  Prints one JSON line.

    python scripts/bench_gradient.py --qubits 28 --layers 2 --repeats 10
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
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--mode", choices=["fused", "pergate"], default="fused")
    args = ap.parse_args()
    if args.repeats < 10:
        ap.error("--repeats must be at least 10")

    import numpy as np
    import qsim_amd as q

    n = args.qubits
    mode = q.RunMode.Fused if args.mode == "fused" else q.RunMode.PerGate
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
    sim = q.Simulator(n, mode)

    def a_run():
        sim.run(circuit)
        sim.synchronize()

    def b_fused():
        os.environ.pop("QSIM_ADJOINT_FUSED", None)  # (read by the engine at every call)
        return sim.gradient(circuit, h, mode)

    def c_unfused():
        os.environ["QSIM_ADJOINT_FUSED"] = "0"
        try:
            return sim.gradient(circuit, h, mode)
        finally:
            os.environ.pop("QSIM_ADJOINT_FUSED", None)

    shift_k = [0]

    def d_pair():
        k = shift_k[0] % P
        shift_k[0] += 1
        e = []
        for sign in (1.0, -1.0):
            th = angles.copy()
            th[k] += sign * np.pi / 2
            sim.run(ansatz(th))
            e.append(sim.expectation(h))
        return (e[0] - e[1]) / 2

    cases = [("a_forward_run", a_run), ("b_gradient_fused", b_fused), ("c_gradient_unfused", c_unfused),
             ("d_parameter_shift_pair", d_pair)]
    for _ in range(2):  # warm-up, excluded (plans, work buffers, first-run layout)
        for _, fn in cases:
            fn()
    times = {name: [] for name, _ in cases}
    for _ in range(args.repeats):
        for name, fn in cases:
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    out = {"bench": "gradient", "qubits": n, "layers": args.layers, "parameters": P, "gates": len(circuit.getGates()),
           "terms": len(h), "mode": args.mode, "repeats": args.repeats, "device": q.device_info(0)["name"],
           "relabeled": sim.state.perm() != list(range(n))}
    for name, _ in cases:
        t = times[name]
        out[name] = {"median_ms": statistics.median(t) * 1e3, "min_ms": min(t) * 1e3, "max_ms": max(t) * 1e3,
                     "spread_max_over_min": max(t) / min(t)}
    a, b, c = (out[k]["median_ms"] for k in ("a_forward_run", "b_gradient_fused", "c_gradient_unfused"))
    d = P * out["d_parameter_shift_pair"]["median_ms"]
    out["d_parameter_shift_total_ms"] = d  # P x the median pair
    out["b_over_a"] = b / a
    out["c_over_b"] = c / b
    out["d_over_b"] = d / b
    print(json.dumps(out))


if __name__ == "__main__":
    main()
