"""Child process of tests/test_dm_pass_matrix_gpu.py (and, with --plan-only, of
tests/test_dm_pass_matrix_cpu.py): the density-matrix pass matrix (tests/dm_pass_cases.py) under
one set of knobs that the library reads once per process (QSIM_JIT_XOR_DIAG, QSIM_TILE_RB,
QSIM_TILE_R0, QSIM_DM_RELABEL_MIN_BITS), which the parent has put into this process's environment.

    python tests/dm_pass_child.py 3 [--plan-only]     (the index into dm_pass_cases.CHILDREN)

prints one JSON line {"cases": N, "worst": x, "failures": [...], "missing": [...], "per_config": {...}}.
--plan-only plans the same circuits on the host and runs nothing (no GPU needed; a relabeled
configuration only has its cases planned under identity labels there: the labels it is about exist
after a first run on the device, and the GPU run checks its required classes under them).  Exit
status 1 on any failure or missing class."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "cuda-quantum-simulator_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("QSIM_CACHE", "0")


def planned(dc, qsim, s):
    """(circuits, classes) as the host plans configuration s under identity labels."""
    n = s["n"]
    if s.get("jit"):
        picked = dc.generated_circuits(qsim, s)
        todo = [(case, info) for _, case, info in picked]
    else:
        todo = [(case, dc.plan_info(qsim, n, case)) for case in dc.cases(s)]
    hit = set()
    for case, info in todo:
        keys = dc.classes_of(info, n, case[1])
        hit |= keys
        if s.get("jit"):
            assert all(p["ops"] <= 192 for p in info["passes"]), case[0]  # jit.hip kJitMaxOps
            if not s["relabeled"] and any(k[-1] in ("xor_thr", "xor_out") for k in keys):
                # the knob took effect: a triple under a thread-bit or tile-constant control is emitted
                # as per-lane factor pairs exactly when Gen::xor_diag is on
                factors = dc.xor_factor_lines(dc.jit_source(qsim, n, case))
                off = os.environ.get("QSIM_JIT_XOR_DIAG") == "0"
                assert bool(factors) != off, (case[0], "QSIM_JIT_XOR_DIAG", off, len(factors))
    return len(todo), hit


def main(argv):
    import dm_pass_cases as dc
    import qsim_amd
    from qsim_amd import plan

    plan_only = "--plan-only" in argv
    idx = [int(a) for a in argv if not a.startswith("--")]
    out = {"cases": 0, "worst": 0.0, "failures": [], "missing": [], "per_config": {}}
    if len(idx) != 1 or (not plan_only and qsim_amd.device_count() < 1):
        out["failures"] = ["no variant given or no GPU visible"]
        print(json.dumps(out))
        return 1
    try:
        for s in dc.CHILDREN[idx[0]]:
            dc.apply_settings(plan, s)
            plan.set_jit(2 if s.get("jit") else 0, 0 if s.get("jit") else -1)
            need = dc.required(s)
            if s.get("jit") and not plan_only and not s["relabeled"]:
                planned(dc, qsim_amd, s)  # (its source check)
            if plan_only:
                if s["relabeled"]:  # the labels exist on the device only: the GPU run checks coverage
                    need = []
                ran, hit = planned(dc, qsim_amd, dict(s, relabeled=False))
                w, bad = 0.0, []
            elif s["relabeled"]:
                ran, w, bad, hit = dc.run_relabeled(qsim_amd, s, jit=bool(s.get("jit")))
                need = dc.required_relabeled(s)
            elif s.get("jit"):
                ran, w, bad, hit = dc.run_generated(qsim_amd, s)
            else:
                ran, w, bad, hit = dc.run_matrix(qsim_amd, s)
            out["cases"] += ran
            out["worst"] = max(out["worst"], w)
            out["per_config"][s["name"]] = [ran, w]
            out["failures"] += bad
            out["missing"] += [repr(m) for m in dc.missing(need, hit)]
            if bad:  # nothing more on the GPU after a failing size
                break
    finally:
        dc.restore_settings(plan)
        plan.set_jit(1, 20)
    print(json.dumps(out))
    return 1 if out["failures"] or out["missing"] else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
