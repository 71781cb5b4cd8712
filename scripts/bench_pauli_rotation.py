#!/usr/bin/env python3
"""Timing of Pauli-string rotations (csrc/hip/pauli_rot.hip) against what a caller had before.

After a warm-up of every case, the median, minimum and maximum of --repeats synchronised calls
(host clock around calls that end in a stream synchronise; the cases alternate inside every
repeat, each on the state the case before left) of

  a  per-gate RX on logical qubit n - 1 (the existing kernel: the same bytes as one rotation);
     its physical bit under the state's layout is reported as top_qubit_physical [before, after]
  b  applyPauliRotation of weight 1 on the same qubit
  c  one weight-n/2 mixed X / Y / Z string (every second qubit)
  d  the string of c as its textbook decomposition (basis changes, CNOT ladder, RZ) through a
     fused run()
  e  n nearest-neighbour ZZ rotations (a ring) as one applyPauliRotations: one pauli_phase pass
  f  the same n ZZ rotations as CNOT RZ CNOT through a fused run()
  g  one order-2 Trotter step of the transverse-field Ising H (evolve)
  h  pauliGradient of four such steps; against it 2 x count evaluations of applyPauliRotations +
     expectation (the parameter shift a caller had before): one evaluation is timed per repeat and
     h_shift_total = 2 x count x its median (the full 2 x count evaluations are not all executed).

Prints one JSON line per qubit count.

    python scripts/bench_pauli_rotation.py --qubits 24 28 --repeats 10
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-quantum-simulator_amd"))


def bench(q, n, repeats):
    from qsim_amd.observable import trotter_sequence
    from qsim_amd.plan import pauli_rotation_plan

    theta = 0.37
    sim = q.Simulator(n)
    prep = q.Circuit(n)
    for k in range(n):
        prep.h(k)
    sim.run(prep)
    sim.synchronize()

    rx = q.GateOp(q.GateType.Rx, [n - 1], theta)
    letters = {k: "XYZ"[(k // 2) % 3] for k in range(0, n, 2)}
    ladder = sorted(letters)

    decomposed = q.Circuit(n)
    for k in ladder:  # to the Z basis
        if letters[k] == "X":
            decomposed.h(k)
        elif letters[k] == "Y":
            decomposed.sdag(k).h(k)
    for a, b in zip(ladder, ladder[1:]):
        decomposed.cnot(a, b)
    decomposed.rz(ladder[-1], theta)
    for a, b in reversed(list(zip(ladder, ladder[1:]))):
        decomposed.cnot(a, b)
    for k in ladder:
        if letters[k] == "X":
            decomposed.h(k)
        elif letters[k] == "Y":
            decomposed.h(k).s(k)

    zz = q.PauliSum(n)
    zz_circuit = q.Circuit(n)
    for k in range(n):
        a, b = k, (k + 1) % n
        zz.add(theta + 0.01 * k, {a: "Z", b: "Z"})
        zz_circuit.cnot(a, b).rz(b, theta + 0.01 * k).cnot(a, b)

    tfim = q.PauliSum(n)
    for k in range(n - 1):
        tfim.add(-1.0, {k: "Z", k + 1: "Z"})
    for k in range(n):
        tfim.add(-0.7, {k: "X"})
    four_steps = trotter_sequence(tfim, 0.4, 4, 2)
    count = len(four_steps)

    def a_rx():
        sim.applyGate(rx)
        sim.synchronize()

    def b_rot1():
        sim.applyPauliRotation({n - 1: "X"}, theta)
        sim.synchronize()

    def c_string():
        sim.applyPauliRotation(letters, theta)
        sim.synchronize()

    def d_string_decomposed():
        sim.run(decomposed)
        sim.synchronize()

    def e_zz_phase():
        sim.applyPauliRotations(zz)
        sim.synchronize()

    def f_zz_decomposed():
        sim.run(zz_circuit)
        sim.synchronize()

    def g_trotter_step():
        sim.evolve(tfim, 0.1, 1, 2)
        sim.synchronize()

    def h_gradient():
        return sim.pauliGradient(four_steps, tfim)

    def h_shift_evaluation():
        sim.applyPauliRotations(four_steps)
        return sim.expectation(tfim)

    cases = [("a_rx_per_gate", a_rx), ("b_rotation_weight1", b_rot1), ("c_rotation_half_weight", c_string),
             ("d_string_decomposed_fused", d_string_decomposed), ("e_zz_one_phase_pass", e_zz_phase),
             ("f_zz_decomposed_fused", f_zz_decomposed), ("g_trotter2_step", g_trotter_step),
             ("h_pauli_gradient", h_gradient), ("h_shift_evaluation", h_shift_evaluation)]
    for _ in range(2):  # warm-up, excluded (plans, work buffers, first-run layout)
        for _, fn in cases:
            fn()
    # (a)-(c) address LOGICAL qubit n - 1: the fused runs of the warm-up may have relabeled the
    # state, so the physical bit the three cases pair over is recorded, before and after the timing
    top_before = sim.state.perm()[n - 1]
    times = {name: [] for name, _ in cases}
    for _ in range(repeats):
        for name, fn in cases:
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    out = {"bench": "pauli_rotation", "qubits": n, "repeats": repeats, "device": q.device_info(0)["name"],
           "string_weight": len(letters), "decomposed_gates": decomposed.getGateCount(),
           "zz_rotations": len(zz), "zz_plan": pauli_rotation_plan(zz), "zz_decomposed_gates": zz_circuit.getGateCount(),
           "trotter_step_plan": pauli_rotation_plan(trotter_sequence(tfim, 0.1, 1, 2)),
           "gradient_rotations": count, "relabeled": sim.state.perm() != list(range(n)),
           "top_qubit_physical": [top_before, sim.state.perm()[n - 1]]}
    for name, _ in cases:
        t = times[name]
        out[name] = {"median_ms": statistics.median(t) * 1e3, "min_ms": min(t) * 1e3, "max_ms": max(t) * 1e3,
                     "spread_max_over_min": max(t) / min(t)}
    med = {name: out[name]["median_ms"] for name, _ in cases}
    out["b_over_a"] = med["b_rotation_weight1"] / med["a_rx_per_gate"]
    out["c_over_a"] = med["c_rotation_half_weight"] / med["a_rx_per_gate"]
    out["d_over_c"] = med["d_string_decomposed_fused"] / med["c_rotation_half_weight"]
    out["f_over_e"] = med["f_zz_decomposed_fused"] / med["e_zz_one_phase_pass"]
    out["h_shift_total_ms"] = 2 * count * med["h_shift_evaluation"]  # 2 x count x the median evaluation
    out["h_shift_over_gradient"] = out["h_shift_total_ms"] / med["h_pauli_gradient"]
    state_bytes = 16.0 * (1 << n)
    out["a_GBps"] = 2 * state_bytes / med["a_rx_per_gate"] / 1e6
    out["b_GBps"] = 2 * state_bytes / med["b_rotation_weight1"] / 1e6
    out["c_GBps"] = 2 * state_bytes / med["c_rotation_half_weight"] / 1e6
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--qubits", type=int, nargs="+", default=[24, 28])
    ap.add_argument("--repeats", type=int, default=10)
    args = ap.parse_args()
    if args.repeats < 10:
        ap.error("--repeats must be at least 10")
    import qsim_amd as q
    for n in args.qubits:
        print(json.dumps(bench(q, n, args.repeats)), flush=True)


if __name__ == "__main__":
    main()
