#!/usr/bin/env python3
"""Timing of the batched sweep gradient (BatchedSimulator.gradientSweep) against the two ways to get
per-member gradients without it.

The workload is the layered ansatz of scripts/bench_batch_sweep.py (per layer: Ry and Rz on every
qubit, then a CNOT ladder; --layers of them, default 4) at one angle set per member, with the
transverse-field Ising Pauli sum as the energy.  One step is, from |0...0>,

  gradient  reset + gradientSweep(circuit, angles[B, P], H): B energies and B x P gradients
  loop      B times reset + Simulator.gradient(circuit_t, H): the adjoint method member by member
  shift     exact parameter shift through the sweep: for each of the P slots, reset +
            runSweep(angles with that column + pi/2) + getExpectations(H), and the same with - pi/2
            (every slot of the ansatz is an Rx / Ry / Rz, for which the rule is exact)
  sweep     reset + runSweep(circuit, angles) + getExpectations(H): the energies alone, for scale

Every step ends in a synchronising readout, so the host wall clock around it is the device time plus
the launch path a caller pays.  Per variant: --warmup untimed steps, then the median / min / max of
--steps timed ones (--baseline-steps for loop and shift, whose steps take seconds).  One further,
untimed, profiled gradientSweep gives the time and the algorithmic bytes of the step kernel
(batch_adjoint_step, 128 B per amplitude pair) and with them its achieved bytes/s.

Writes one JSON line per shape (also printed) to --out.

    python scripts/bench_batch_gradient.py --out profiles/batch_gradient/bench_batch_gradient.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-quantum-simulator_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_batch_sweep import ansatz, ising  # noqa: E402


def timed(step, steps, warmup):
    for _ in range(warmup):
        step()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        step()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "steps": steps}


def bench(q, n, B, layers, steps, warmup, baseline_steps):
    from qsim_amd.plan import batch_gradient_plan, parameterised_slots
    P = 2 * n * layers
    rng = np.random.default_rng(1234 + n)
    angles = rng.uniform(-np.pi, np.pi, size=(B, P))
    circuit = ansatz(q, n, layers, angles[0])
    slots = parameterised_slots(circuit)
    H = ising(q, n)
    info = batch_gradient_plan(circuit, B, H)
    batch = q.BatchedSimulator(n, B, noise=q.BatchedNoise.Physical)

    def gradient():
        batch.reset()
        return batch.gradientSweep(circuit, angles, H)

    def sweep():
        batch.reset()
        batch.runSweep(circuit, angles)
        return batch.getExpectations(H)

    def shift():
        g = np.empty((B, P))
        for k in range(P):
            e = []
            for d in (np.pi / 2, -np.pi / 2):
                a = angles.copy()
                a[:, k] += d
                batch.reset()
                batch.runSweep(circuit, a)
                e.append(batch.getExpectations(H))
            g[:, k] = (e[0] - e[1]) / 2
        return g

    sim = q.Simulator(n)
    members = [ansatz(q, n, layers, angles[t]) for t in range(B)]

    def loop():
        v, g = np.empty(B), np.empty((B, P))
        for t in range(B):
            sim.reset()
            v[t], gt = sim.gradient(members[t], H)
            g[t] = np.asarray(gt)[slots]
        return v, g

    # the three routes compute the same numbers
    (v_b, g_b), (v_l, g_l), g_s = gradient(), loop(), shift()
    err_loop = float(max(np.abs(v_b - v_l).max(), np.abs(g_b - g_l).max()))
    err_shift = float(np.abs(g_b - g_s).max())
    assert err_loop < 1e-9 and err_shift < 1e-9, (err_loop, err_shift)
    r_grad = timed(gradient, steps, warmup)
    r_sweep = timed(sweep, steps, warmup)
    r_loop = timed(loop, baseline_steps, 0)  # (the agreement check above was its warm-up)
    r_shift = timed(shift, baseline_steps, 0)
    batch.profile(True)
    gradient()
    stats = {s["name"]: s for s in batch.profileStats()}
    batch.profile(False)
    st = stats["batch_adjoint_step"]
    return {"bench": "batch_gradient", "n": n, "batch": B, "layers": layers, "slots": P, "gates": len(circuit.getGates()),
            "segments": info["segments"], "apply_launches": info["apply_launches"], "work_bytes": info["work_bytes"],
            "warmup": warmup, "gradient": r_grad, "sweep": r_sweep, "loop": r_loop, "shift": r_shift,
            "loop_over_gradient": r_loop["median_ms"] / r_grad["median_ms"],
            "shift_over_gradient": r_shift["median_ms"] / r_grad["median_ms"],
            "gradient_over_sweep": r_grad["median_ms"] / r_sweep["median_ms"],
            "step_kernel": {"launches": st["launches"], "ms": st["ms"], "alg_bytes": st["alg_bytes"],
                            "gbytes_per_s": st["alg_bytes"] / (st["ms"] * 1e-3) / 1e9},
            "profile_ms": {k: v["ms"] for k, v in sorted(stats.items())},
            "max_diff_vs_loop": err_loop, "max_diff_vs_shift": err_shift}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["16x256", "20x16"], help="qubits x members")
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--baseline-steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import qsim_amd as q
    lines = []
    for shape in args.shapes:
        n, B = (int(v) for v in shape.split("x"))
        r = bench(q, n, B, args.layers, args.steps, args.warmup, args.baseline_steps)
        print(json.dumps(r), flush=True)
        lines.append(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
