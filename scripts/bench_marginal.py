#!/usr/bin/env python3
"""Timing of the marginal / reduced-density-matrix readout (csrc/hip/marginal.hip) against what a
caller had before.

The state is what a fused run of W-HC (random {H, CNOT}, depth 100, seed 42) leaves, so a
non-identity qubit layout is in place.  Every case is timed with a pair of HIP events recorded on
the state's stream around the synchronising call (so the figure is the call as the stream sees it,
device-to-host copy of the result included), median / min / max of --repeats calls after --warmup
warm-up calls; the host wall clock of the same calls is kept beside it.

  marginal_k{1,8,16,20}_{low,high,mixed}  marginalProbabilities, the selected qubits on the lowest /
        highest / alternating low-high PHYSICAL positions (mapped back through the layout)
  rdm_k{2,4,6}_{low,high,mixed}           reducedDensityMatrix; flops = 8 * 2^k * 2^n (all of rho is
        accumulated), GFLOP/s from the event time
  total_probability                       getTotalProbability(): the same 16 B/amplitude read
  probabilities_numpy_k8                  getProbabilities() + a numpy marginal of 8 qubits: what a
        user does today (restores the layout; the state is re-run before each call so every call
        pays what a first reader pays)

Prints one JSON line per qubit count.

    python scripts/bench_marginal.py --qubits 26 28
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-quantum-simulator_amd"))


class Events:
    """A pair of HIP events on one stream (the runtime the engine already loaded)."""

    def __init__(self, stream):
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.stream = ctypes.c_void_p(stream)
        self.a, self.b = ctypes.c_void_p(), ctypes.c_void_p()
        for e in (self.a, self.b):
            assert self.hip.hipEventCreate(ctypes.byref(e)) == 0

    def time_ms(self, fn):
        assert self.hip.hipEventRecord(self.a, self.stream) == 0
        t0 = time.perf_counter()
        fn()
        wall = time.perf_counter() - t0
        assert self.hip.hipEventRecord(self.b, self.stream) == 0
        assert self.hip.hipEventSynchronize(self.b) == 0
        ms = ctypes.c_float()
        assert self.hip.hipEventElapsedTime(ctypes.byref(ms), self.a, self.b) == 0
        return ms.value, wall * 1e3


def numpy_marginal(p, n, qubits):
    t = p.reshape((2,) * n)
    keep = [n - 1 - q for q in reversed(qubits)]
    drop = tuple(a for a in range(n) if a not in keep)
    return np.transpose(t.sum(axis=drop), np.argsort(np.argsort(keep))).reshape(-1)


def bench(q, n, repeats, warmup):
    from qsim_amd.plan import marginal_plan
    circuit = q.createRandomHCCircuit(n, 100, 42)
    sim = q.Simulator(n)
    sim.run(circuit)
    sim.synchronize()
    perm = sim.state.perm()
    inv = [perm.index(p) for p in range(n)]  # physical position -> logical qubit
    ev = Events(sim.state.stream())

    def where(k, kind):
        if kind == "low":
            pos = list(range(k))
        elif kind == "high":
            pos = list(range(n - k, n))
        else:  # alternately from the bottom and from the top
            pos = [i // 2 if i % 2 == 0 else n - 1 - i // 2 for i in range(k)]
        return [inv[p] for p in pos]

    cases = []
    for k in (1, 8, 16, 20):
        for kind in ("low", "high", "mixed"):
            qs = where(k, kind)
            cases.append((f"marginal_k{k}_{kind}", qs, False, lambda qs=qs: sim.marginalProbabilities(qs)))
    for k in (2, 4, 6):
        for kind in ("low", "high", "mixed"):
            qs = where(k, kind)
            cases.append((f"rdm_k{k}_{kind}", qs, True, lambda qs=qs: sim.reducedDensityMatrix(qs)))
    cases.append(("total_probability", None, False, lambda: sim.state.getTotalProbability()))

    out = {"bench": "marginal", "qubits": n, "repeats": repeats, "warmup": warmup,
           "device": q.device_info(0)["name"], "relabeled": perm != list(range(n)),
           "layout": sim.state.layoutInfo(), "state_GiB": 16.0 * (1 << n) / 2 ** 30}
    for name, qs, rdm, fn in cases:
        for _ in range(warmup):
            fn()
        t = [ev.time_ms(fn) for _ in range(repeats)]
        e = [x[0] for x in t]
        rec = {"event_median_ms": statistics.median(e), "event_min_ms": min(e), "event_max_ms": max(e),
               "wall_median_ms": statistics.median(x[1] for x in t),
               "GBps": 16.0 * (1 << n) / statistics.median(e) / 1e6}
        if qs is not None:
            rec["plan"] = marginal_plan(n, qs, perm, rdm=rdm)
        if rdm:
            rec["GFLOPps"] = 8.0 * (1 << len(qs)) * (1 << n) / statistics.median(e) / 1e6
        out[name] = rec
    assert sim.state.perm() == perm, "a reader restored the layout"

    # what a user does today: all 2^n probabilities to the host, reduced there
    qs8 = where(8, "mixed")
    t = []
    for i in range(warmup + repeats):
        sim.reset()
        sim.run(circuit)
        sim.synchronize()
        got = ev.time_ms(lambda: numpy_marginal(sim.getProbabilities(), n, qs8))
        if i >= warmup:
            t.append(got)
    out["probabilities_numpy_k8"] = {"event_median_ms": statistics.median(x[0] for x in t),
                                     "wall_median_ms": statistics.median(x[1] for x in t),
                                     "wall_min_ms": min(x[1] for x in t), "wall_max_ms": max(x[1] for x in t)}
    base = out["total_probability"]["event_median_ms"]
    out["marginal_over_total_probability"] = {name: out[name]["event_median_ms"] / base
                                              for name, _, rdm, _ in cases if name.startswith("marginal")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--qubits", type=int, nargs="+", default=[26, 28])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if args.repeats < 10 or args.warmup < 3:
        ap.error("--repeats must be at least 10 and --warmup at least 3")
    import qsim_amd as q
    for n in args.qubits:
        print(json.dumps(bench(q, n, args.repeats, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
