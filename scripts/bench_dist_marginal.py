#!/usr/bin/env python3
"""Timing of marginal probabilities and reduced density matrices on the sharded state
(csrc/hip/dist_marginal.hip) with --world virtual ranks on one GPU, against the single-GPU readers
(csrc/hip/marginal.hip) on the same state.

After one W-HC run (createRandomHCCircuit) at --qubits qubits, the median, minimum and maximum of
--repeats synchronised calls (host clock around calls that end in a stream synchronise; the first
call of every case is excluded as warm-up; the cases alternate inside every repeat) of

  a  getTotalProbability() of the sharded state
  b  a marginal of 8 qubits on local positions, and one with the rank positions among the 8
  c  the same two marginals through Simulator.marginalProbabilities (the single-GPU baseline)
  d  matrices of k = 2, 4 and 6 qubits on local positions only
  e  matrices of the same k with 1 and with 3 rank positions among them (1 and 7 cross steps)
  f  getProbabilities() + numpy for the 8 qubits of b (--gather-repeats calls; it gathers 2^n
     doubles on the host)

Qubits are picked by PHYSICAL position through perm() after the run.  On virtual ranks a
"transfer" is a device copy that competes with the kernels for the same HBM: e against d says
nothing about a link between GPUs.  Prints one JSON line.

    python scripts/bench_dist_marginal.py --qubits 28 --world 8 --repeats 12
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
    ap.add_argument("--gather-repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=42)
    args = ap.parse_args()
    if args.repeats < 10:
        ap.error("--repeats must be at least 10")

    import numpy as np
    import qsim_amd as q
    from qsim_amd.dist import DistributedSimulator, marginal_plan

    n, world = args.qubits, args.world
    g = world.bit_length() - 1
    L = n - g
    if g != 3 or L < 16:
        ap.error("needs world 8 and at least 19 qubits")
    circuit = q.createRandomHCCircuit(n, args.depth, args.seed)
    d = DistributedSimulator.virtual(n, world)
    d.run(circuit)
    d.synchronize()
    sim = q.Simulator(n)
    sim.run(circuit)
    sim.synchronize()
    perm = d.perm()
    inv = {p: lq for lq, p in enumerate(perm)}
    logical = lambda positions: [inv[p] for p in positions]

    # physical positions: lane, wave, per-thread and run-choosing bits; the top local one left out
    local8 = [0, 3, 6, 9, 12, 14, L - 3, L - 2]
    rank8 = local8[:5] + [L, L + 1, L + 2]
    local_k = {2: [1, 13], 4: [1, 7, 10, 13], 6: [1, 4, 7, 10, 13, L - 2]}
    sels = {"b_marginal8_local": (local8, False), "b_marginal8_rank3": (rank8, False)}
    for k, pos in local_k.items():
        sels[f"d_rdm{k}_local"] = (pos, True)
        sels[f"e_rdm{k}_rank1"] = (pos[:k - 1] + [L], True)
        if k > 2:
            sels[f"e_rdm{k}_rank3"] = (pos[:k - 3] + [L, L + 1, L + 2], True)
    plans = {name: marginal_plan(n, world, perm, logical(pos), rdm) for name, (pos, rdm) in sels.items()}
    assert plans["b_marginal8_local"]["k_rank"] == 0 and plans["b_marginal8_rank3"]["k_rank"] == 3
    assert plans["e_rdm6_rank3"]["cross_steps"] == 7 and plans["e_rdm6_rank1"]["pair_rule"] == 1

    def reader(pos, rdm):
        qs = logical(pos)
        return (lambda: d.reducedDensityMatrix(qs)) if rdm else (lambda: d.marginalProbabilities(qs))

    cases = [("a_total_probability", d.getTotalProbability)]
    cases += [(name, reader(pos, rdm)) for name, (pos, rdm) in sels.items()]
    cases += [("c_marginal8_local_single_gpu", lambda: sim.marginalProbabilities(logical(local8))),
              ("c_marginal8_rank3_single_gpu", lambda: sim.marginalProbabilities(logical(rank8)))]
    cases += [(f"c_rdm{k}_local_single_gpu", (lambda qs: lambda: sim.reducedDensityMatrix(qs))(logical(pos)))
              for k, pos in local_k.items()]

    def gathered():
        p = d.getProbabilities().reshape((2,) * n)
        qs = logical(rank8)
        rest = tuple(n - 1 - b for b in range(n) if b not in qs)
        m = p.sum(axis=rest)                                   # axes left: descending qubit index
        order = sorted(qs, reverse=True)
        return np.transpose(m, [order.index(b) for b in reversed(qs)]).reshape(-1)

    out = {"bench": "dist_marginal", "qubits": n, "world": world, "virtual": True, "depth": args.depth,
           "repeats": args.repeats, "gather_repeats": args.gather_repeats, "device": q.device_info(0)["name"],
           "relabeled": perm != list(range(n)), "plans": plans,
           "positions": {name: pos for name, (pos, _) in sels.items()}}
    values = {name: fn() for name, fn in cases}                # warm-up, excluded
    times = {name: [] for name, _ in cases}
    for _ in range(args.repeats):                              # cases alternate inside every repeat
        for name, fn in cases:
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    times["f_get_probabilities_numpy"] = []
    for _ in range(args.gather_repeats):
        t0 = time.perf_counter()
        values["f_get_probabilities_numpy"] = gathered()
        times["f_get_probabilities_numpy"].append(time.perf_counter() - t0)
    for name, t in times.items():
        med = statistics.median(t)
        out[name] = {"median_ms": med * 1e3, "min_ms": min(t) * 1e3, "max_ms": max(t) * 1e3,
                     "spread_max_over_min": max(t) / min(t), "state_bytes_per_s": 16.0 * (1 << n) / med}
    ratio = lambda a, b: out[a]["median_ms"] / out[b]["median_ms"]
    out["b_local_over_c"] = ratio("b_marginal8_local", "c_marginal8_local_single_gpu")
    out["b_rank3_over_c"] = ratio("b_marginal8_rank3", "c_marginal8_rank3_single_gpu")
    for k in local_k:
        out[f"d_rdm{k}_over_single_gpu"] = ratio(f"d_rdm{k}_local", f"c_rdm{k}_local_single_gpu")
        out[f"e_rdm{k}_rank1_over_d"] = ratio(f"e_rdm{k}_rank1", f"d_rdm{k}_local")
    out["f_over_b_rank3"] = ratio("f_get_probabilities_numpy", "b_marginal8_rank3")
    for a, b in (("b_marginal8_local", "c_marginal8_local_single_gpu"),
                 ("b_marginal8_rank3", "c_marginal8_rank3_single_gpu"),
                 ("b_marginal8_rank3", "f_get_probabilities_numpy")):
        assert np.max(np.abs(values[a] - values[b])) <= 1e-12, (a, b)
    for k in local_k:
        assert np.max(np.abs(values[f"d_rdm{k}_local"] - values[f"c_rdm{k}_local_single_gpu"])) <= 1e-12
    assert d.perm() == perm, "a reader changed the qubit map"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
