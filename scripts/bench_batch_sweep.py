#!/usr/bin/env python3
"""Timing of a batched parameter sweep (BatchedSimulator.runSweep) against its two yardsticks.

The workload is a layered ansatz (per layer: Ry and Rz on every qubit, then a CNOT ladder;
--layers of them, default 4) evaluated at one angle set per member, followed by the per-member
energy of a transverse-field Ising Pauli sum.  One step is, from |0...0>,

  sweep     reset + runSweep(circuit, angles[B, P]) + getExpectations(H)          (this change)
  shared    reset + run(circuit) + getExpectations(H) on the same object: one angle set for all
            members, noise-free — the same passes with shared matrices, i.e. the ceiling
  loop      B times reset + Simulator.run(circuit_t) + expectation(H): what a user does today

Every step ends in a synchronising readout, so the host wall clock around it is the device time
plus the launch path a caller pays.  Per variant: --warmup steps (plans, layouts, first launches),
then — because circuit-specialised pass kernels are compiled in the background — further untimed
steps until specialised passes have arrived and their number stands still (at most --settle
seconds: a variant that gets none waits that long), then the median / min / max of --steps timed
steps; jit_passes in the result says how many passes of the last step ran specialised kernels.

Writes one JSON line per shape (also printed) to --out.

    python scripts/bench_batch_sweep.py --out profiles/batch_sweep/bench_batch_sweep.jsonl
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


def ansatz(q, n, layers, angles):
    c = q.Circuit(n)
    a = iter(angles)
    for _ in range(layers):
        for k in range(n):
            c.ry(k, float(next(a)))
        for k in range(n):
            c.rz(k, float(next(a)))
        for k in range(n - 1):
            c.cnot(k, k + 1)
    return c


def ising(q, n):
    h = q.PauliSum(n)
    for k in range(n - 1):
        h.add(1.0, {k: "Z", k + 1: "Z"})
    for k in range(n):
        h.add(0.5, {k: "X"})
    return h


def timed(step, steps, warmup, settle_s, jit_passes):
    for _ in range(warmup):
        step()
    t_end = time.perf_counter() + settle_s
    seen, stable = jit_passes(), 0
    # until specialised kernels have arrived and their number has stood still for 10 steps; a variant
    # that never gets one (every pass of a sweep may hold a member-dependent gate) waits settle_s
    while time.perf_counter() < t_end and not (seen > 0 and stable >= 10):
        step()
        now = jit_passes()
        stable = stable + 1 if now == seen else 0
        seen = now
        time.sleep(0.05)
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        step()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "jit_passes": jit_passes()}


def bench(q, n, B, layers, steps, warmup, settle_s):
    from qsim_amd.plan import batch_sweep_plan
    P = 2 * n * layers
    rng = np.random.default_rng(1234 + n)
    angles = rng.uniform(-np.pi, np.pi, size=(B, P))
    circuit = ansatz(q, n, layers, angles[0])
    H = ising(q, n)
    info = batch_sweep_plan(circuit, B)
    batch = q.BatchedSimulator(n, B, noise=q.BatchedNoise.Physical)

    def sweep():
        batch.reset()
        batch.runSweep(circuit, angles)
        return batch.getExpectations(H)

    def shared():
        batch.reset()
        batch.run(circuit)
        return batch.getExpectations(H)

    sim = q.Simulator(n)
    members = [ansatz(q, n, layers, angles[t]) for t in range(B)]

    def loop():
        out = np.empty(B)
        for t in range(B):
            sim.reset()
            sim.run(members[t])
            out[t] = sim.expectation(H)
        return out

    # the three variants compute the same energies (loop: member by member)
    e_sweep, e_loop = sweep(), loop()
    err = float(np.abs(e_sweep - e_loop).max())
    assert err < 1e-9, f"sweep and loop energies differ by {err}"
    assert abs(shared()[B - 1] - e_loop[0]) < 1e-9
    r_sweep = timed(sweep, steps, warmup, settle_s, lambda: batch.lastRunInfo()[1])
    r_shared = timed(shared, steps, warmup, settle_s, lambda: batch.lastRunInfo()[1])
    r_loop = timed(loop, steps, max(1, warmup // 2), settle_s, lambda: sim.state.lastRunInfo()[1])
    return {"bench": "batch_sweep", "n": n, "batch": B, "layers": layers, "slots": P, "gates": len(circuit.getGates()),
            "passes": info["passes"], "member_passes": info["member_passes"], "table_bytes": info["table_bytes"],
            "steps": steps, "warmup": warmup, "sweep": r_sweep, "shared": r_shared, "loop": r_loop,
            "sweep_over_shared": r_sweep["median_ms"] / r_shared["median_ms"],
            "loop_over_sweep": r_loop["median_ms"] / r_sweep["median_ms"],
            "max_energy_diff_sweep_vs_loop": err}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["16x256", "20x16"], help="qubits x members")
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--settle", type=float, default=10.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.steps < 10:
        ap.error("--steps must be at least 10")
    import qsim_amd as q
    lines = []
    for shape in args.shapes:
        n, B = (int(v) for v in shape.split("x"))
        r = bench(q, n, B, args.layers, args.steps, args.warmup, args.settle)
        print(json.dumps(r), flush=True)
        lines.append(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
