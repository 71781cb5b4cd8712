#!/usr/bin/env python3
"""Timing of Pauli-string rotations on the sharded state (csrc/hip/dist_pauli_rot.hip) on virtual
ranks of one GPU, with the protocol of scripts/bench_dist_gradient.py.

After a warm-up of every case, the median, minimum and maximum of --repeats synchronised calls
(host clock; the cases alternate inside every repeat) of one rotation per class, each against the
single-GPU Simulator.applyPauliRotation of the same string at the same qubit count:

  phase  a run of 8 Z-only strings, Z factors on rank positions among them
  local  X / Y / Z factors, the X and Y ones on local positions, a Z on a rank position
  cross  the local string with its X moved to a rank position: one whole-shard transfer per rank
  cross_ladder  the cross string decomposed for run(): basis changes, a CNOT ladder, Rz, and back
                (what a caller of the sharded simulator had before), on a state of its own and
                re-written before every call so that its X sits on a rank position again: run()
                remaps that qubit local and leaves it there

then one order-2 Trotter step of the transverse-field Ising chain (evolve) and a pauliGradient of
that step's sequence against the chain itself, sharded and single, and the per-kernel times of one
profiled sharded gradient call.  The strings are chosen by physical position under the map two
W-HC runs leave.  On virtual ranks every transfer is a device copy that competes with the kernels
for the same HBM: these are kernel rates, nothing about xGMI follows from them.  Prints one JSON
line.

    python scripts/bench_dist_pauli_rotation.py --qubits 28 --world 8 --repeats 10
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
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--skip-single", action="store_true", help="leave the single-GPU cases out (memory)")
    args = ap.parse_args()
    if args.repeats < 10:
        ap.error("--repeats must be at least 10")

    import qsim_amd as q
    from qsim_amd.dist import DistributedSimulator, pauli_gradient_plan, pauli_rotation_plan
    from qsim_amd.dist import plan as dist_plan
    from qsim_amd.observable import trotter_sequence

    n, world = args.qubits, args.world
    L = n - (world.bit_length() - 1)
    d = DistributedSimulator.virtual(n, world)
    ladder_d = DistributedSimulator.virtual(n, world)  # (run() remaps: it keeps a state of its own)
    hc = q.createRandomHCCircuit(n, 100, 42)
    for _ in range(2):
        d.run(hc)
        ladder_d.run(hc)
    perm = d.perm()
    inv = {p: k for k, p in enumerate(perm)}
    at = lambda p: inv[p]  # the logical qubit at physical position p
    sim = None if args.skip_single else q.Simulator(n)

    phase = q.PauliSum(n)
    for k in range(8):
        phase.add(0.1 * (k + 1), {at(k): "Z", at(L - 1 - k): "Z", at(L + k % (n - L)): "Z"})
    local = {at(L - 1): "X", at(3): "Y", at(0): "Z", at(n - 1): "Z"}
    cross = {at(n - 1): "X", at(3): "Y", at(0): "Z", at(L - 1): "Z"}
    theta = 0.37

    def ladder(factors):
        c = q.Circuit(n)
        qs = sorted(factors)
        for k in qs:
            if factors[k] == "X":
                c.h(k)
            elif factors[k] == "Y":
                c.sdag(k).h(k)
        for a, b in zip(qs, qs[1:]):
            c.cnot(a, b)
        c.rz(qs[-1], theta)
        for a, b in reversed(list(zip(qs, qs[1:]))):
            c.cnot(a, b)
        for k in qs:
            if factors[k] == "X":
                c.h(k)
            elif factors[k] == "Y":
                c.h(k).s(k)
        return c

    # run() brings the rank-position qubit local and leaves it there, so a repeat of the same
    # circuit would no longer cross ranks: before every call (untimed) the string is written again
    # by position under the map the last call left, its X on the top rank position once more
    ladder_circuit = [None]

    def ladder_prepare():
        pinv = {p: k for k, p in enumerate(ladder_d.perm())}
        ladder_circuit[0] = ladder({pinv[n - 1]: "X", pinv[3]: "Y", pinv[0]: "Z", pinv[L - 1]: "Z"})

    tfim = q.PauliSum(n)
    for k in range(n - 1):
        tfim.add(-1.0, {k: "Z", k + 1: "Z"})
    for k in range(n):
        tfim.add(-0.7, {k: "X"})
    step = trotter_sequence(tfim, 0.1, 1, 2)

    def synced(obj, fn):
        def run():
            fn()
            obj.synchronize()
        return run

    cases = [("dist_phase", synced(d, lambda: d.applyPauliRotations(phase))),
             ("dist_local", synced(d, lambda: d.applyPauliRotation(local, theta))),
             ("dist_cross", synced(d, lambda: d.applyPauliRotation(cross, theta))),
             ("dist_cross_ladder", synced(ladder_d, lambda: ladder_d.run(ladder_circuit[0]))),
             ("dist_trotter_step", synced(d, lambda: d.evolve(tfim, 0.1, 1, 2))),
             ("dist_gradient", lambda: d.pauliGradient(step, tfim))]
    if sim is not None:
        cases += [("single_phase", synced(sim, lambda: sim.applyPauliRotations(phase))),
                  ("single_local", synced(sim, lambda: sim.applyPauliRotation(local, theta))),
                  ("single_cross", synced(sim, lambda: sim.applyPauliRotation(cross, theta))),
                  ("single_trotter_step", synced(sim, lambda: sim.evolve(tfim, 0.1, 1, 2))),
                  ("single_gradient", lambda: sim.pauliGradient(step, tfim))]
    prepare = {"dist_cross_ladder": ladder_prepare}
    for _ in range(2):  # warm-up, excluded (tables, work shards, plans)
        for name, fn in cases:
            prepare.get(name, lambda: None)()
            fn()
    times = {name: [] for name, _ in cases}
    ladder_remaps = []
    for _ in range(args.repeats):
        for name, fn in cases:
            prepare.get(name, lambda: None)()
            if name == "dist_cross_ladder":
                ladder_remaps.append(sum(s["kind"] == "exchange" for s in
                                         dist_plan(ladder_circuit[0], world, 0, ladder_d.perm())[0]))
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    d.profile(True)
    d.pauliGradient(step, tfim)
    stats = d.profileStats()
    d.profile(False)
    out = {"bench": "dist_pauli_rotation", "qubits": n, "world": world, "virtual": True, "repeats": args.repeats,
           "device": q.device_info(0)["name"], "perm": perm,
           "plan_phase": pauli_rotation_plan(n, world, perm, phase),
           "plan_local": pauli_rotation_plan(n, world, perm, q.PauliSum(n).add(theta, local)),
           "plan_cross": pauli_rotation_plan(n, world, perm, q.PauliSum(n).add(theta, cross)),
           "plan_gradient": pauli_gradient_plan(n, world, perm, step, tfim),
           "ladder_gates": len(ladder_circuit[0].getGates()), "ladder_remaps_per_call": ladder_remaps,
           "trotter_rotations": len(step),
           "profile_one_gradient": stats}
    for name, _ in cases:
        t = times[name]
        out[name] = {"median_ms": statistics.median(t) * 1e3, "min_ms": min(t) * 1e3, "max_ms": max(t) * 1e3,
                     "spread_max_over_min": max(t) / min(t)}
    amp_bytes = 16.0 * (1 << n)
    out["dist_local_gbps"] = 2 * amp_bytes / out["dist_local"]["median_ms"] / 1e6   # 32 B per amplitude
    out["dist_cross_gbps"] = 3 * amp_bytes / out["dist_cross"]["median_ms"] / 1e6   # 48 B, the copy apart
    out["ladder_over_cross"] = out["dist_cross_ladder"]["median_ms"] / out["dist_cross"]["median_ms"]
    if sim is not None:
        for k in ("phase", "local", "cross", "trotter_step", "gradient"):
            out[f"{k}_dist_over_single"] = out[f"dist_{k}"]["median_ms"] / out[f"single_{k}"]["median_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
