#!/usr/bin/env python3
"""Timing of Pauli-sum expectation values on the sharded state (csrc/hip/dist_expect.hip) with
--world virtual ranks on one GPU, against the single-GPU kernels on the same number of bytes.

After one W-HC run (createRandomHCCircuit) at --qubits qubits, the median, minimum and maximum of
--repeats synchronised calls (host clock around calls that end in a stream synchronise; the first
call of every case is excluded as warm-up; the cases alternate inside every repeat) of

  a  getTotalProbability() of the sharded state
  b  64 Z-only terms                               (one read of every shard, no transfer)
  c  one string with X on a local qubit            (one pair pass inside every shard)
  d  one string with X on a rank qubit             (half of every shard moves, then one pass)
  e  a transverse-field Ising H: n ZZ + n X terms  (1 + n passes, one transfer per rank qubit)
  f  case e with QSIM_DIST_EXPECT_OVERLAP=0        (one receive buffer, every transfer waited for)
  g  case e on a plain Simulator at the same size  (the single-GPU kernels)
  h  case b, i  case c on that Simulator

Qubits are picked by PHYSICAL position through perm() after the run.  On virtual ranks a
"transfer" is a device copy that competes with the kernels for the same HBM: d / c and e / f say
nothing about a link between GPUs.  Prints one JSON line.

    python scripts/bench_dist_expectation.py --qubits 28 --world 8 --repeats 12
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
    ap.add_argument("--depth", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--seed", type=int, default=42)
    args = ap.parse_args()
    if args.repeats < 10:
        ap.error("--repeats must be at least 10")

    import numpy as np
    import qsim_amd as q
    from qsim_amd.dist import DistributedSimulator, expectation_plan

    n, world = args.qubits, args.world
    L = n - (world.bit_length() - 1)
    circuit = q.createRandomHCCircuit(n, args.depth, args.seed)
    d = DistributedSimulator.virtual(n, world)
    d.run(circuit)
    d.synchronize()
    sim = q.Simulator(n)
    sim.run(circuit)
    sim.synchronize()
    perm = d.perm()
    inv = {p: lq for lq, p in enumerate(perm)}
    rng = np.random.default_rng(args.seed)

    diag64 = q.PauliSum(n)
    seen = set()
    while len(seen) < 64:
        f = tuple(int(b) for b in np.nonzero(rng.integers(0, 2, size=n))[0])
        if f and f not in seen:
            seen.add(f)
            diag64.add(float(rng.uniform(-1, 1)), {b: "Z" for b in f})
    x_local = q.PauliSum(n).add(1.0, {inv[L // 2]: "X", inv[0]: "Z"})
    x_rank = q.PauliSum(n).add(1.0, {inv[L]: "X", inv[0]: "Z"})
    ising = q.PauliSum(n)
    for k in range(n):
        ising.add(1.0, {k: "Z", (k + 1) % n: "Z"})
        ising.add(0.5, {k: "X"})
    plans = {name: expectation_plan(n, world, perm, h) for name, h in
             (("b", diag64), ("c", x_local), ("d", x_rank), ("e", ising))}
    assert plans["b"]["transfers"] == 0 and plans["c"]["transfers"] == 0 and plans["d"]["transfers"] == 1

    def serial():
        os.environ["QSIM_DIST_EXPECT_OVERLAP"] = "0"  # (read by the engine at every call)
        try:
            return d.expectation(ising)
        finally:
            os.environ.pop("QSIM_DIST_EXPECT_OVERLAP", None)

    cases = [
        ("a_total_probability", 1, d.getTotalProbability),
        ("b_64_z_terms", 1, lambda: d.expectation(diag64)),
        ("c_x_on_local_qubit", 1, lambda: d.expectation(x_local)),
        ("d_x_on_rank_qubit", 1, lambda: d.expectation(x_rank)),
        ("e_ising", n + 1, lambda: d.expectation(ising)),
        ("f_ising_no_overlap", n + 1, serial),
        ("g_ising_single_gpu", n + 1, lambda: sim.expectation(ising)),
        ("h_64_z_terms_single_gpu", 1, lambda: sim.expectation(diag64)),
        ("i_x_on_local_qubit_single_gpu", 1, lambda: sim.expectation(x_local)),
    ]
    out = {"bench": "dist_expectation", "qubits": n, "world": world, "virtual": True, "depth": args.depth,
           "repeats": args.repeats, "device": q.device_info(0)["name"],
           "relabeled": perm != list(range(n)), "plans": plans}
    values = {}
    for name, _, fn in cases:
        values[name] = fn()  # warm-up, excluded
    times = {name: [] for name, _, _ in cases}
    for _ in range(args.repeats):  # cases alternate inside every repeat
        for name, _, fn in cases:
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    for name, passes, _ in cases:
        t = times[name]
        med = statistics.median(t)
        out[name] = {"median_ms": med * 1e3, "min_ms": min(t) * 1e3, "max_ms": max(t) * 1e3,
                     "spread_max_over_min": max(t) / min(t), "passes": passes,
                     "bytes_per_s": 16.0 * (1 << n) * passes / med, "value": values[name]}
    g_pass = out["g_ising_single_gpu"]["median_ms"] / (n + 1)
    out["g_ms_per_pass"] = g_pass
    out["b_over_g_pass"] = out["b_64_z_terms"]["median_ms"] / g_pass
    out["c_over_g_pass"] = out["c_x_on_local_qubit"]["median_ms"] / g_pass
    out["b_over_h"] = out["b_64_z_terms"]["median_ms"] / out["h_64_z_terms_single_gpu"]["median_ms"]
    out["c_over_i"] = out["c_x_on_local_qubit"]["median_ms"] / out["i_x_on_local_qubit_single_gpu"]["median_ms"]
    out["d_bytes_moved"] = plans["d"]["bytes_sent_per_rank"] * world
    out["e_over_g"] = out["e_ising"]["median_ms"] / out["g_ising_single_gpu"]["median_ms"]
    out["f_over_e"] = out["f_ising_no_overlap"]["median_ms"] / out["e_ising"]["median_ms"]
    tol = 1e-12 * 1.5 * n
    assert abs(values["e_ising"] - values["g_ising_single_gpu"]) <= tol
    assert abs(values["e_ising"] - values["f_ising_no_overlap"]) <= tol
    assert d.perm() == perm, "an expectation call changed the qubit map"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
