#!/usr/bin/env python3
"""Timing of the Pauli-sum expectation values (csrc/hip/expect.hip) against the norm reduction.

After one W-HC run (createRandomHCCircuit) at --qubits qubits, the median, minimum and maximum of
--repeats synchronised calls (host clock around calls that end in a stream synchronise; the first
call of every case is excluded as warm-up) of

  a  getTotalProbability()                     (reads the same 16 B per amplitude)
  b  one Z-string term
  c  one term with x != 0
  d  64 diagonal terms in one call             (one pass over the state)
  e  the same 64 terms as 64 calls
  f  a 100-term sum with 10 distinct x masks   (10 passes)
  d_plain  case d with QSIM_EXPECT_SPLIT=0     (the kernel without the z lane/run split)

Prints one JSON line.  bytes_per_s of a case: 16 B x 2^n x its passes over the median.

    python scripts/bench_expectation.py --qubits 28 --repeats 12
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
    ap.add_argument("--depth", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--seed", type=int, default=42)
    args = ap.parse_args()
    if args.repeats < 10:
        ap.error("--repeats must be at least 10")

    import numpy as np
    import qsim_amd as q

    n = args.qubits
    sim = q.Simulator(n)
    sim.run(q.createRandomHCCircuit(n, args.depth, args.seed))
    sim.synchronize()
    perm = sim.state.perm()
    rng = np.random.default_rng(args.seed)

    def rand_z():
        return {int(b): "Z" for b in np.nonzero(rng.integers(0, 2, size=n))[0]}

    one_z = q.PauliSum(n).add(1.0, rand_z() or {0: "Z"})
    one_x = q.PauliSum(n).add(1.0, {0: "X", n // 2: "Y", n - 1: "X", 3: "Z"})
    diag_terms = []
    while len(diag_terms) < 64:
        f = rand_z()
        if f and f not in diag_terms:
            diag_terms.append(f)
    diag64 = q.PauliSum(n)
    singles = []
    for f in diag_terms:
        c = float(rng.uniform(-1, 1))
        diag64.add(c, f)
        singles.append(q.PauliSum(n).add(c, f))
    mixed = q.PauliSum(n)
    xs = [{}] + [{int(b): "X" for b in rng.choice(n, size=3, replace=False)} for _ in range(9)]
    for t in range(100):
        f = dict(xs[t % 10])
        for b, l in rand_z().items():
            f[b] = "Y" if f.get(b) == "X" else ("Z" if b not in f else f[b])
        mixed.add(float(rng.uniform(-1, 1)), f)

    def e_loop():
        total = 0.0
        for s in singles:
            total += sim.expectation(s)
        return total

    def d_plain():
        os.environ["QSIM_EXPECT_SPLIT"] = "0"  # (read by the engine at every call)
        try:
            return sim.expectation(diag64)
        finally:
            os.environ.pop("QSIM_EXPECT_SPLIT", None)

    cases = [
        ("a_total_probability", 1, sim.state.getTotalProbability),
        ("b_one_z_term", 1, lambda: sim.expectation(one_z)),
        ("c_one_x_term", 1, lambda: sim.expectation(one_x)),
        ("d_64_diagonal_one_call", 1, lambda: sim.expectation(diag64)),
        ("e_64_diagonal_64_calls", 64, e_loop),
        ("f_100_terms_10_x_masks", 10, lambda: sim.expectation(mixed)),
        ("d_plain_64_diagonal_one_call", 1, d_plain),
    ]
    out = {"bench": "expectation", "qubits": n, "depth": args.depth, "repeats": args.repeats,
           "device": q.device_info(0)["name"], "relabeled": perm != list(range(n))}
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
    out["d_vs_e_speedup"] = out["e_64_diagonal_64_calls"]["median_ms"] / out["d_64_diagonal_one_call"]["median_ms"]
    out["d_split_vs_plain_speedup"] = (out["d_plain_64_diagonal_one_call"]["median_ms"] /
                                       out["d_64_diagonal_one_call"]["median_ms"])
    assert values["d_plain_64_diagonal_one_call"] == values["d_64_diagonal_one_call"]
    assert sim.state.perm() == perm, "an expectation call changed the qubit layout"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
