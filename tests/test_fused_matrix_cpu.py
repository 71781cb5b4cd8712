"""CPU: the fused-pass operand-class matrix (tests/fused_cases.py) before any GPU time is spent.

  * every case of every in-process configuration of tests/test_fused_matrix_gpu.py plans the way
    it says (a per-gate step only where the case expects one, the pass shape the size rules give)
    and the classes hit cover fused_cases.required in full;
  * the same for the variants that need a process of their own, planned in child processes
    (tests/fused_child.py --plan-only), and for the circuits chosen for the generated kernels;
  * plan.plan_exec_host, the host mirror of the staged kernels' index math, equals the dense
    reference on dense states for every case, which validates cases, reference and masks;
  * circuits wider than one tile have a relayout plan whose passes move qubits; its host
    execution, and the host play of the run-sharing cycle, equal the dense reference from dense
    states;
  * the circuit of more than 512 H plans as one pass at the kMaxUnnormH cap;
  * plan.plan_stage_info names every gate exactly once, in plan_fused's order.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fused_cases as fc


@pytest.fixture
def plan(qsim):
    from qsim_amd import plan
    yield plan
    fc.restore_settings(plan)


@pytest.mark.parametrize("s", fc.IN_PROCESS, ids=lambda s: s["name"])
def test_cases_plan_as_built_and_cover_required(qsim, plan, s):
    fc.apply_settings(plan, s)
    shape, hit, n_single = fc.shape(s), set(), 0
    case_list = fc.cases(s)
    for label, gates, single in case_list:
        assert 1 <= len(gates) - (9 if s["anchor"] else 0) <= 6, label
        info = plan.plan_stage_info(fc.circuit_of(qsim, s["n"], gates))
        hit |= fc.classes_of(info)
        got = any(p["single"] for p in info["passes"])
        n_single += got
        if single is not None:
            assert got == single, (s["name"], label, "per-gate step", got)
        for p in info["passes"]:
            if p["single"]:
                continue
            demoted = s["anchor"] and (p["h"], p["rb"]) == (6, 4)  # (a second pass of an anchored case)
            assert (p["h"], p["rb"], p["r0"]) == shape or demoted, (s["name"], label, p)
    missing = fc.missing(fc.required(s), hit)
    print(f"{s['name']}: {len(case_list)} cases ({n_single} with a per-gate step), {len(hit)} classes, "
          f"{len(fc.required(s))} required")
    assert not missing, (s["name"], missing)


@pytest.mark.parametrize("s", [c for c in fc.NATURAL + fc.CTRL_OUT_OFF[:1] if c["n"] >= 10],
                         ids=lambda s: s["name"])
def test_host_mirror_equals_dense_reference(qsim, plan, s):
    """plan_exec_host mode 0 plans at h = min(6, n - 6) with the default stage width.  (No case
    has a relayout plan: each acts inside one tile; see test_relayout_plans_from_dense_states.)"""
    fc.apply_settings(plan, s)
    n, worst = s["n"], 0.0
    for k, (label, gates, _) in enumerate(fc.cases(s)):
        c = fc.circuit_of(qsim, n, gates)
        psi = fc.dense_state(n, 1000 * n + k)
        want, _ = fc.reference(n, psi, gates)
        got, _, _ = plan.plan_exec_host(c, mode=0, state=psi)
        worst = max(worst, _err(got, want))
        assert worst <= fc.TOL, (s["name"], label, worst)
    print(f"{s['name']}: worst component error {worst:.3e}")


def _err(got, want):
    return float(max(np.max(np.abs(got.real - want.real)), np.max(np.abs(got.imag - want.imag))))


@pytest.mark.parametrize("s", fc.GENERATED, ids=lambda s: s["name"])
def test_generated_circuits_cover_required(qsim, plan, s):
    """The few circuits picked for the generated kernels: every pass within the 192 ops a generated
    pass may hold (jit.hip kJitMaxOps), none per-gate, at least one of several stages."""
    fc.apply_settings(plan, s)
    picked = fc.generated_circuits(qsim, s)
    hit, multi = set(), 0
    for label, gates, info in picked:
        hit |= fc.classes_of(info)
        for p in info["passes"]:
            assert not p["single"] and p["rb"] > 0 and p["ops"] <= 192, (s["name"], label, p)
            multi += p["stages"] >= 2
    print(f"{s['name']}: {len(picked)} circuits, {len(hit)} classes")
    assert 1 <= len(picked) <= 20 and multi >= 1
    assert not fc.missing(fc.required(s), hit)


@pytest.mark.parametrize("seed", [0, 1])
def test_relayout_plans_from_dense_states(qsim, plan, seed):
    n = 16
    plan.set_relabel(1, n)
    plan.set_relayout(1, n)
    plan.set_run_share(1, 4)
    gates = fc.relayout_circuit(n, seed)
    assert len({t for t, _, _ in gates}) == 17  # every gate type
    c = fc.circuit_of(qsim, n, gates)
    passes = plan.plan_relayout(c)[1]
    assert passes >= 2
    info = plan.plan_stage_info(c, relayout=True)
    assert len(info["passes"]) == passes and all(p["relayout"] and p["stages"] >= 2 for p in info["passes"])
    assert sorted(r["src"] for r in info["ops"] if r["src"] >= 0) == list(range(len(gates)))
    psi = fc.dense_state(n, 77 + seed)
    want, _ = fc.reference(n, psi, gates)
    got, perm, ran = plan.plan_exec_host(c, mode=1, state=psi)
    assert ran == passes and perm != list(range(n))
    print(f"seed {seed}: {passes} relayout passes, worst component error {_err(got, want):.3e}")
    assert _err(got, want) <= fc.TOL
    # the run-sharing cycle of the GPU test: six identical runs, four of them calls of the joint plan
    joint, single, _ = plan.plan_share_info(c, 4)
    assert 0 < joint < 4 * single
    for _ in range(5):
        want, _ = fc.reference(n, want, gates)
    got, launched, pending = plan.plan_share_host(c, 6, 4, state=psi)
    assert sum(launched[2:]) == joint and pending[-1] == 0
    assert _err(got, want) <= fc.TOL


@pytest.mark.subprocess
def test_child_variants_plan_and_cover_required():
    """The knobs of fused_cases.CHILDREN are read once per process, so each variant is planned in a
    child (no GPU): its cases, or for the generated-kernel variants its chosen circuits, cover
    fused_cases.required under that variant's planner."""
    here = os.path.dirname(os.path.abspath(__file__))
    base = {k: v for k, v in os.environ.items() if k not in fc.KNOBS}
    for idx, variant in enumerate(fc.CHILDREN):
        env = dict(base, **{k: str(v) for k, v in variant[0]["env"].items()})
        r = subprocess.run([sys.executable, os.path.join(here, "fused_child.py"), str(idx), "--plan-only"],
                           capture_output=True, text=True, timeout=120, env=env)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert lines, (variant[0]["name"], r.returncode, r.stderr[-3000:])
        out = json.loads(lines[-1])
        assert r.returncode == 0 and out["missing"] == [] and out["failures"] == [], (variant[0]["name"], out)
        if variant[0].get("jit"):
            assert out["cases"] >= 2 and out["jit_passes"] >= out["cases"] and out["multi_stage"] >= 1, out
        else:
            assert out["cases"] == sum(len(fc.cases(s)) for s in variant)


def test_many_h_circuit_plans_one_pass_at_the_cap(qsim, plan):
    gates = fc.many_h_circuit()
    assert sum(t == fc.H for t, _, _ in gates) == 600
    last = {}
    for t, qs, _ in gates:  # no two H adjacent on a qubit
        assert not (t == fc.H and last.get(qs[0]) == fc.H)
        last[qs[0]] = t
    info = plan.plan_stage_info(fc.circuit_of(qsim, 12, gates))
    assert len(info["passes"]) == 1 and not info["passes"][0]["single"]
    assert info["passes"][0]["hu_count"] == 512
    m1 = [r for r in info["ops"] if r["kind"] == fc.K_M1]
    assert len(m1) == 600
    assert sum(r["sub"] == fc.S_H for r in m1) == 512 and sum(r["sub"] == fc.S_GEN for r in m1) == 88


@pytest.mark.parametrize("n", [6, 9, 10, 11, 21])
def test_introspection_covers_every_gate_in_plan_order(qsim, plan, n):
    """Sizes where plan_fused(c, hmax) and a run use the same stage width (unstaged tiles, h = 4,
    5, and 12-qubit tiles above 20 qubits)."""
    c = qsim.createRandomCircuit(n, 120, 5 + n)
    c.swap(0, n - 1).toffoli(1, n - 1, 3).swap(2, 4)
    order, pass_of, _ = plan.plan_fused(c, hmax=min(6, n - 6))
    info = plan.plan_stage_info(c)
    src = [r["src"] for r in info["ops"] if r["src"] >= 0]
    assert sorted(src) == list(range(c.getGateCount()))
    assert src == [int(g) for g in order]
    assert sum(r["src"] < 0 for r in info["ops"]) == 2 * sum(
        1 for r in info["ops"] if r["src"] >= 0 and c.getGates()[r["src"]].type == fc.SWAP
        and not info["passes"][r["pass"]]["single"] and info["passes"][r["pass"]]["rb"] > 0)
    assert [p for p in pass_of if p >= 0] == sorted(p for p in pass_of if p >= 0)
    for p in info["passes"]:
        assert p["lds_fixed"] + p["lds_searched"] == max(0, p["stages"] - 1) == len(p["swizzle"])
