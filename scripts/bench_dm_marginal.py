#!/usr/bin/env python3
"""Timing of the density-matrix subset readers and the fidelity on the device
(csrc/hip/dm_marginal.hip) against purity() and against the host route.

DensityMatrixSimulator at each of --qubits, the W-HC circuit (createRandomHCCircuit) with
depolarizing --noise on all qubits, one fused run from a reset rho (so rho lies under relabeled index
bits).  Median, minimum and maximum of --repeats synchronised calls after two warm-ups (host clock
around calls that end in a stream synchronise), the cases alternating inside every repeat, of

  marginal  marginalProbabilities of 4 qubits            (reads 2^n elements)
  rdm       reducedDensityMatrix of 6 qubits             (reads 2^(n+6) elements)
  fidelity  fidelity(psi), psi a fixed random vector     (streams all 4^n elements)
  purity    purity() on the same rho: the existing reader that streams the same 16 * 4^n bytes, the
            yardstick for fidelity

and, --host-repeats times, the host route a caller had before: getMatrix() (which restores the
identity layout and copies 4^n elements; every call follows a fresh reset + run, not timed) plus the
numpy reduction of each reader.  Prints one JSON line.

    python scripts/bench_dm_marginal.py --qubits 12 13 14
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-quantum-simulator_amd"))


def summary(t):
    return {"median_ms": statistics.median(t) * 1e3, "min_ms": min(t) * 1e3, "max_ms": max(t) * 1e3}


def timed(fn):
    t0 = time.perf_counter()
    v = fn()
    return time.perf_counter() - t0, v


def bench_one(q, np, n, args):
    dim = 1 << n
    c = q.createRandomHCCircuit(n, args.depth, args.seed)
    nm = q.NoiseModel()
    nm.addDepolarizingAll(n, args.noise)
    sim = q.DensityMatrixSimulator(n, nm)
    sv = sim.density.state
    marg_q = [1, 4, 7, 10]
    rdm_q = [0, 1, 2, 3, 4, 5]
    rng = np.random.default_rng(args.seed)
    psi = rng.normal(size=dim) + 1j * rng.normal(size=dim)
    psi /= np.linalg.norm(psi)

    def fresh_run():
        sim.reset()
        sim.run(c)
        sv.synchronize()

    fresh_run()  # (the first run chooses the index-bit labels; later ones reuse them)
    layout, perm = sv.layoutInfo(), sv.perm()
    cases = {"marginal": lambda: sim.marginalProbabilities(marg_q), "rdm": lambda: sim.reducedDensityMatrix(rdm_q),
             "fidelity": lambda: sim.fidelity(psi), "purity": sim.getPurity}
    times = {k: [] for k in cases}
    values = {}
    for rep in range(2 + args.repeats):
        for name, fn in cases.items():
            t, values[name] = timed(fn)
            if rep >= 2:
                times[name].append(t)
    assert sv.perm() == perm, "a reader changed the index-bit layout"

    def host_marginal(m):
        p = np.real(np.diagonal(m)).reshape((2,) * n)  # axis x is qubit n - 1 - x
        keep = [n - 1 - k for k in reversed(marg_q)]
        return np.transpose(p, keep + [a for a in range(n) if a not in keep]).reshape(1 << len(marg_q), -1).sum(axis=1)

    def host_rdm(m):  # the six lowest qubits: the low 6 bits of both indices
        t = m.reshape(dim >> 6, 64, dim >> 6, 64)
        return np.einsum("biba->ia", t)

    host = {k: [] for k in ("get_matrix", "marginal", "rdm", "fidelity")}
    checks = {}
    for _ in range(args.host_repeats):
        fresh_run()
        t_get, m = timed(sim.getDensityMatrix)
        host["get_matrix"].append(t_get)
        for name, fn in (("marginal", host_marginal), ("rdm", host_rdm),
                         ("fidelity", lambda mm: float(np.vdot(psi, mm @ psi).real))):
            t, checks[name] = timed(lambda: fn(m))
            host[name].append(t_get + t)
        del m
    assert np.abs(checks["marginal"] - values["marginal"]).max() < 1e-9
    assert np.abs(checks["rdm"] - values["rdm"]).max() < 1e-9
    assert abs(checks["fidelity"] - values["fidelity"]) < 1e-9

    out = {"qubits": n, "relabeled": layout["relabeled"], "elements_of_rho": dim * dim,
           "elements_read": {"marginal": dim, "rdm": dim << 6, "fidelity": dim * dim},
           "device": {k: summary(t) for k, t in times.items()}, "host": {k: summary(t) for k, t in host.items()},
           "fidelity_value": values["fidelity"], "purity_value": values["purity"]}
    out["fidelity_over_purity"] = out["device"]["fidelity"]["median_ms"] / out["device"]["purity"]["median_ms"]
    out["fidelity_gb_per_s"] = 16.0 * dim * dim / (out["device"]["fidelity"]["median_ms"] * 1e-3) / 1e9
    for k in ("marginal", "rdm", "fidelity"):
        out[f"host_over_device_{k}"] = out["host"][k]["median_ms"] / out["device"][k]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--qubits", type=int, nargs="+", default=[12, 13, 14])
    ap.add_argument("--depth", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--noise", type=float, default=0.01)
    args = ap.parse_args()
    if args.repeats < 10:
        ap.error("--repeats must be at least 10")
    if min(args.qubits) < 11:
        ap.error("--qubits must be at least 11 (the marginal's qubits go up to 10)")

    import numpy as np
    import qsim_amd as q

    out = {"bench": "dm_marginal", "depth": args.depth, "noise": args.noise, "repeats": args.repeats,
           "host_repeats": args.host_repeats, "device": q.device_info(0)["name"],
           "results": [bench_one(q, np, n, args) for n in args.qubits]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
