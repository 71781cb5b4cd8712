#!/usr/bin/env python3
"""Timing of the overlap (Gram) matrix of a batched ensemble (BatchedSimulator.overlapMatrix)
against the route it replaces and a bandwidth yardstick.

The ensemble is prepared once per shape by a layered-ansatz sweep (per layer: Ry and Rz on every
qubit, then a CNOT ladder; --layers of them, one angle set per member) and then only read:

  mfma      overlapMatrix()                                       (the matrix-core tile kernel)
  fma       overlapMatrix() with QSIM_OVERLAP_MFMA=0              (the same tiles with plain FMAs)
  readback  B x getStateVector + numpy conj(A) @ A.T              (existing API only: the route today)
  expect    getExpectations of a single-Z observable: one streaming pass over the same bytes

Every variant ends in a synchronising readout, so the host wall clock around a call is the device
time plus the launch path and the copy of the result.  mfma and fma are timed alternately, call by
call, after --warmup calls of each; the median / min / max of --steps calls are kept (readback:
--readback-steps).  A second, profiled pass (per-launch device events, qsim_batch_profile) gives
the tile and the reduction kernels' own times; the FLOP figures divide by the tile kernel's time:

  useful_flops   entries computed (B (B + 1) / 2 of the Hermitian half) x 2^n x 8 (four real FMAs)
  issued_flops   tiles launched x 64 x 64 x 2^n x 8 (what the tile grid multiplies, padding included)

Writes one JSON line per shape (also printed) to --out.

    python scripts/bench_batch_overlap.py --out profiles/batch_overlap/bench_batch_overlap.jsonl
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_batch_sweep import ansatz  # noqa: E402


def _summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "calls": len(ms)}


def _clock(f):
    t0 = time.perf_counter()
    out = f()
    return (time.perf_counter() - t0) * 1e3, out


def _component_diff(a, b):
    d = a - b
    return float(max(np.abs(d.real).max(), np.abs(d.imag).max()))


def bench(q, n, B, layers, steps, warmup, readback_steps):
    from qsim_amd.plan import batch_overlap_plan
    P = 2 * n * layers
    angles = np.random.default_rng(1234 + n).uniform(-np.pi, np.pi, size=(B, P))
    batch = q.BatchedSimulator(n, B, noise=q.BatchedNoise.Physical)
    batch.runSweep(ansatz(q, n, layers, angles[0]), angles)
    info = batch_overlap_plan(n, B)
    Z = q.PauliSum(n)
    Z.add(1.0, {0: "Z"})

    def overlap(mfma):
        os.environ["QSIM_OVERLAP_MFMA"] = "1" if mfma else "0"
        try:
            return batch.overlapMatrix()
        finally:
            del os.environ["QSIM_OVERLAP_MFMA"]

    def readback():
        A = np.array([batch.getStateVector(t) for t in range(B)])
        return A.conj() @ A.T

    # the routes agree (bound: 2 * 2^(n+1) * 2^-53 per component for unit vectors)
    g_mfma, g_fma, g_host = overlap(True), overlap(False), readback()
    bound = 2.0 * 2.0 ** (n + 1) * 2.0 ** -53 * 1.001
    worst = max(_component_diff(g_mfma, g_host), _component_diff(g_fma, g_host))
    assert worst < bound, f"overlapMatrix and the readback route differ by {worst}"

    for _ in range(warmup):
        overlap(True)
        overlap(False)
        batch.getExpectations(Z)
    t_mfma, t_fma, t_exp = [], [], []
    for _ in range(steps):  # alternating: both see the same machine
        t_mfma.append(_clock(lambda: overlap(True))[0])
        t_fma.append(_clock(lambda: overlap(False))[0])
        t_exp.append(_clock(lambda: batch.getExpectations(Z))[0])
    t_read = [_clock(readback)[0] for _ in range(readback_steps)]

    # kernel times, in a pass of their own (per-launch events)
    batch.profile(True)
    for _ in range(steps):
        overlap(True)
        overlap(False)
    stats = {s["name"]: s for s in batch.profileStats() if s["name"].startswith("batch_overlap")}
    batch.profile(False)
    kern = {k: v["ms"] / v["launches"] for k, v in stats.items()}
    K = float(1 << n)
    useful = (B * (B + 1) // 2) * K * 8.0
    issued = info["tiles"] * 64.0 * 64.0 * K * 8.0
    state_bytes = B * K * 16.0
    r = {"bench": "batch_overlap", "n": n, "batch": B, "layers": layers, "plan": info, "steps": steps,
         "warmup": warmup, "mfma": _summary(t_mfma), "fma": _summary(t_fma), "readback": _summary(t_read),
         "expect": _summary(t_exp), "kernel_ms": kern, "state_bytes": state_bytes,
         "useful_flops": useful, "issued_flops": issued, "max_diff_vs_readback": worst}
    r["readback_over_mfma"] = r["readback"]["median_ms"] / r["mfma"]["median_ms"]
    r["fma_over_mfma"] = r["fma"]["median_ms"] / r["mfma"]["median_ms"]
    r["mfma_over_expect"] = r["mfma"]["median_ms"] / r["expect"]["median_ms"]
    for name in ("batch_overlap_mfma", "batch_overlap_vec"):
        if name in kern:
            r[name + "_useful_tflops"] = useful / (kern[name] * 1e-3) / 1e12
            r[name + "_issued_tflops"] = issued / (kern[name] * 1e-3) / 1e12
            r[name + "_operand_tbps"] = state_bytes / (kern[name] * 1e-3) / 1e12
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["16x256", "20x16"], help="qubits x members")
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--readback-steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.steps < 10:
        ap.error("--steps must be at least 10")
    import qsim_amd as q
    lines = []
    for shape in args.shapes:
        n, B = (int(v) for v in shape.split("x"))
        r = bench(q, n, B, args.layers, args.steps, args.warmup, args.readback_steps)
        print(json.dumps(r), flush=True)
        lines.append(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
