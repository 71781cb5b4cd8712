#!/usr/bin/env python3
"""Timing of Re Tr(rho H) on the device (csrc/hip/dm_expect.hip) against the readers that restore
the identity layout first.

DensityMatrixSimulator at --qubits qubits, the W-HC circuit (createRandomHCCircuit) with
depolarizing --noise on all qubits (the dm_14q object of bench.py), H = a periodic transverse-field
Ising chain (n ZZ bonds + n X fields: 1 + n groups).  Median, minimum and maximum of --repeats
synchronised calls after two warm-ups (host clock around calls that end in a stream synchronise) of

  a  expectation(H) under the layout the run left (the state is not touched, so the calls repeat)
  b  getDensityMatrix() + numpy for the same H: what a caller had before.  Every call follows a
     fresh reset + run (not timed), so it pays the layout restore a variational loop pays per step;
     b_identity: the same call once more, the identity layout already restored
  c  getProbabilities() (the canonicalising reader; enough for the Z-only part of H), the same way

and, from per-launch HIP events of one profiled run, the time of one fused pass over rho.  Prints
one JSON line.

    python scripts/bench_dm_expectation.py --qubits 14
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
    ap.add_argument("--qubits", type=int, default=14)
    ap.add_argument("--depth", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--noise", type=float, default=0.01)
    args = ap.parse_args()
    if args.repeats < 10:
        ap.error("--repeats must be at least 10")

    import numpy as np
    import qsim_amd as q

    n = args.qubits
    dim = 1 << n
    c = q.createRandomHCCircuit(n, args.depth, args.seed)
    nm = q.NoiseModel()
    nm.addDepolarizingAll(n, args.noise)
    sim = q.DensityMatrixSimulator(n, nm)
    sv = sim.density.state
    obs = q.PauliSum(n)
    for k in range(n):
        obs.add(-1.0, {k: "Z", (k + 1) % n: "Z"})
    for k in range(n):
        obs.add(-0.7, {k: "X"})
    terms = obs.terms()
    idx = np.arange(dim)

    def popcount_parity(v):
        par = np.zeros(v.shape, dtype=np.int64)
        while v.any():
            par ^= v & 1
            v = v >> 1
        return par

    def host_value(rho):  # sum_t c_t Re sum_i rho[i][i ^ x] i^nY (-1)^popcount(i & z)
        total = 0.0
        for x, z, coeff in terms:
            phase = 1j ** bin(x & z).count("1")
            total += coeff * float((phase * np.sum(rho[idx, idx ^ x] * (1 - 2 * popcount_parity(idx & z)))).real)
        return total

    def fresh_run():
        sim.reset()
        sim.run(c)
        sv.synchronize()

    fresh_run()  # (the first run chooses the index-bit labels; later ones reuse them)
    sv.profile(True)
    sv.profileReset()
    fresh_run()
    stats = sv.profileStats()
    sv.profile(False)
    passes, _ = sv.lastRunInfo()
    run_ms = sum(s["ms"] for s in stats)
    layout = sv.layoutInfo()
    perm = sv.perm()

    def timed(fn):
        t0 = time.perf_counter()
        v = fn()
        return time.perf_counter() - t0, v

    times = {k: [] for k in ("a", "b", "b_identity", "c", "c_identity")}
    values = {}
    for rep in range(2 + args.repeats):  # cases alternate inside every repeat; two warm-ups
        keep = rep >= 2
        t, values["a"] = timed(lambda: sim.expectation(obs))
        if keep:
            times["a"].append(t)
        assert sv.perm() == perm, "an expectation call changed the index-bit layout"
        for name, fn in (("b", lambda: host_value(sim.getDensityMatrix())), ("c", sim.getProbabilities)):
            t, v = timed(fn)
            t2, _ = timed(fn)
            if name == "b":
                values["b"] = v
            if keep:
                times[name].append(t)
                times[name + "_identity"].append(t2)
            fresh_run()

    out = {"bench": "dm_expectation", "qubits": n, "depth": args.depth, "noise": args.noise,
           "repeats": args.repeats, "device": q.device_info(0)["name"], "terms": len(terms), "groups": 1 + n,
           "elements_read": (1 + n) * dim, "elements_of_rho": dim * dim, "relabeled": layout["relabeled"],
           "run_passes": passes, "run_ms_device": run_ms, "one_pass_ms": run_ms / max(1, passes)}
    for name, t in times.items():
        out[name] = {"median_ms": statistics.median(t) * 1e3, "min_ms": min(t) * 1e3, "max_ms": max(t) * 1e3,
                     "spread_max_over_min": max(t) / min(t)}
    out["value_a"], out["value_b"] = values["a"], values["b"]
    out["b_over_a"] = out["b"]["median_ms"] / out["a"]["median_ms"]
    out["c_over_a"] = out["c"]["median_ms"] / out["a"]["median_ms"]
    out["a_over_one_pass"] = out["a"]["median_ms"] / out["one_pass_ms"]
    assert abs(values["a"] - values["b"]) < 1e-9 * len(terms), (values["a"], values["b"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
