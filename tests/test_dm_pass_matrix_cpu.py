"""CPU: the density-matrix pass matrix (tests/dm_pass_cases.py) before any GPU time is spent.

  * the Kraus / unitary reference of dm_pass_cases equals the oracle's restatement (oracle.dm_run,
    oracle.dm_channel) on random general matrices at 1e-14: every gate type, every channel type,
    reference_y, n = 1..4;
  * every case of every in-process configuration plans into the pass shape the size rules give, and
    the classes hit cover dm_pass_cases.required in full; the same for the variants that need a
    process of their own (tests/dm_pass_child.py --plan-only) and for the circuits chosen for the
    generated kernels, which stay within kJitMaxOps per pass;
  * plan.dm_plan_exec_host, the host mirror of the staged kernels on the lowered density-matrix ops,
    equals the reference at 1e-12 for every case of every staged configuration from 10 index bits,
    each under identity labels and under three random permutations of the 2n index bits: dm_lower, dm_channel, dm_col, dm_row, permute_op and
    the planner's index math for these ops;
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import dm_pass_cases as dc


@pytest.fixture
def plan(qsim):
    from qsim_amd import plan
    yield plan
    dc.restore_settings(plan)


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_kraus_reference_equals_oracle(oracle, n):
    rng = np.random.default_rng(40 + n)
    worst = 0.0
    for t in range(6):
        for q in range(n):
            rho = dc.dense_rho(n, 10 * t + q)
            got, _ = dc.channel(n, rho, t, q, dc.PROB[t])
            worst = max(worst, dc.err_of(got, oracle.dm_channel(rho, n, t, q, dc.PROB[t])))
    types = dc.ONE_Q + ([dc.CNOT, dc.CZ, dc.SWAP] if n > 1 else [])
    for k in range(12):
        gates = []
        for t in (types if k == 0 else [int(x) for x in rng.choice(types, 6)]):
            qs = [int(x) for x in rng.choice(n, 1 if t <= dc.RZ else 2, replace=False)]
            gates.append((t, qs, float(rng.uniform(-3, 3)) if t >= dc.RX and t <= dc.RZ else 0.0))
        channels = [(int(t), int(rng.integers(-1, n)), dc.PROB[int(t)]) for t in rng.permutation(6)[:k % 4]]
        rho = dc.dense_rho(n, 100 + k)
        for ref_y in (False, True):
            got, _ = dc.reference(n, rho, gates, channels, ref_y)
            worst = max(worst, dc.err_of(got, oracle.dm_run(n, gates, channels, rho=rho, reference_y=ref_y)))
    print(f"n={n}: worst component difference {worst:.3e}")
    assert worst <= 1e-14


@pytest.mark.parametrize("s", dc.IN_PROCESS, ids=lambda s: s["name"])
def test_cases_plan_as_built_and_cover_required(qsim, plan, s):
    dc.apply_settings(plan, s)
    shape, hit, n_single, n_demoted, n_kept = dc.shape(s), set(), 0, 0, 0
    case_list = dc.cases(s)
    n_anchor = len(dc.anchor_qubits(s["n"])) if s["anchor"] else 0
    for case in case_list:
        label, gates, channels, _ = case
        assert 1 <= len(gates) - n_anchor <= 6 and len(channels) <= 2, label
        info = dc.plan_info(qsim, s["n"], case)
        hit |= dc.classes_of(info, s["n"], gates)
        n_single += any(p["single"] for p in info["passes"])
        for p in info["passes"]:
            if p["single"]:
                continue
            r0_free = (p["h"], p["rb"]) == shape[:2] and shape[0] >= 4  # (plan_fused picks r0 in 4..6)
            # (h = 7: a pass that fits a 12-bit tile is demoted, one of the unanchored configuration
            # that does not keeps the plan's height)
            mixed = s["h"] == 7 and ((p["h"], p["rb"]) == (6, 4) or p["h"] == 7)
            n_demoted += s["h"] == 7 and (p["h"], p["rb"]) == (6, 4)
            n_kept += s["h"] == 7 and p["h"] == 7
            assert (p["h"], p["rb"], p["r0"]) == shape or r0_free or mixed, (s["name"], label, p)
    if s["name"] == "h7mix_n7":  # the demotion itself: planned at 13 bits, run as a 12-bit tile
        assert n_demoted >= 1 and n_kept >= 1, (n_demoted, n_kept)
    missing = dc.missing(dc.required(s), hit)
    print(f"{s['name']}: {len(case_list)} cases ({n_single} with a per-gate step), {len(hit)} classes, "
          f"{len(dc.required(s))} required")
    assert not missing, (s["name"], missing)


@pytest.mark.parametrize("s", [c for c in dc.IN_PROCESS if 2 * c["n"] >= 10 and dc.shape(c)[1] > 0],
                         ids=lambda s: s["name"])
def test_host_execution_equals_kraus_reference(qsim, plan, s):
    """Every case of every staged configuration from 10 index bits, under identity labels and under
    three random permutations of the 2n index bits (the lowering is the same, the plan is not)."""
    dc.apply_settings(plan, s)
    n, worst, ran = s["n"], 0.0, 0
    rng = np.random.default_rng(7 + n)
    perms = [None] + [[int(b) for b in rng.permutation(2 * n)] for _ in range(3)]
    case_list = dc.cases(s)
    for k, case in enumerate(case_list):
        label, gates, channels, ref_y = case
        rho = dc.dense_rho(n, 1000 * n + k)
        want, _ = dc.reference(n, rho, gates, channels, ref_y)
        c = dc.circuit_of(qsim, n, gates)
        for perm in perms:
            got, _ = plan.dm_plan_exec_host(c, rho, channels, 1 | (dc.REFERENCE_Y if ref_y else 0), perm)
            ran += 1
            err = dc.err_of(got, want)
            worst = max(worst, err)
            assert err <= dc.TOL, (s["name"], label, perm, err)
    print(f"{s['name']}: {ran} host executions, worst component error {worst:.3e}")
    assert ran == 4 * len(case_list)


@pytest.mark.parametrize("s", dc.GENERATED, ids=lambda s: s["name"])
def test_generated_circuits_cover_required(qsim, plan, s):
    """The circuits picked for the generated kernels: every pass staged and within the 192 ops a
    generated pass may hold (jit.hip kJitMaxOps); together they cover required(s), so the xor
    forms, the real 2x2 and the real scales among it."""
    dc.apply_settings(plan, s)
    picked = dc.generated_circuits(qsim, s)
    hit, n_xor, n_factor = set(), 0, 0
    for _, case, info in picked:
        hit |= dc.classes_of(info, s["n"], case[1])
        for p in info["passes"]:
            assert not p["single"] and p["rb"] > 0 and p["ops"] <= 192, (s["name"], case[0], p)
        if any(k[-1] in ("xor_thr", "xor_out") for k in dc.classes_of(info, s["n"], case[1])):
            n_factor += bool(dc.xor_factor_lines(dc.jit_source(qsim, s["n"], case)))
            n_xor += 1
    print(f"{s['name']}: {len(picked)} circuits, {len(hit)} classes")
    assert 1 <= len(picked) <= dc.MAX_GENERATED
    # with Gen::xor_diag on (the default), every circuit with a triple under a thread-bit or
    # tile-constant control carries its per-lane factor pairs; the child with the knob off none
    assert n_xor >= 1 and n_factor == n_xor, (n_xor, n_factor)
    assert not dc.missing(dc.required(s), hit)


@pytest.mark.subprocess
def test_child_variants_plan_and_cover_required():
    here = os.path.dirname(os.path.abspath(__file__))
    base = {k: v for k, v in os.environ.items() if k not in dc.KNOBS}
    for idx, variant in enumerate(dc.CHILDREN):
        env = dict(base, **{k: str(v) for k, v in variant[0]["env"].items()})
        r = subprocess.run([sys.executable, os.path.join(here, "dm_pass_child.py"), str(idx), "--plan-only"],
                           capture_output=True, text=True, timeout=120, env=env)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert lines, (variant[0]["name"], r.returncode, r.stderr[-3000:])
        out = json.loads(lines[-1])
        assert r.returncode == 0 and out["missing"] == [] and out["failures"] == [], (variant[0]["name"], out)
        assert out["cases"] >= len(variant)
