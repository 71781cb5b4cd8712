"""Child process of tests/test_fused_matrix_gpu.py (and, with --plan-only, of
tests/test_fused_matrix_cpu.py): the fused-pass operand matrix under one set of knobs that
fused.hip and jit.hip read once per process (QSIM_TILE_RB, QSIM_TILE_R0, QSIM_FUSED_NT, QSIM_JIT_NT,
QSIM_JIT_PIPE, QSIM_JIT_XCD, QSIM_PLANNER, QSIM_STAGE_SEARCH), which the parent has put into this
process's environment.

    python tests/fused_child.py 3 [--plan-only]     (the index into fused_cases.CHILDREN)

prints one JSON line {"cases": N, "worst": x, "failures": [...], "missing": [...], "jit_passes": k,
"multi_stage": m}: missing lists the patterns of fused_cases.required that the classes hit do not
cover, jit_passes / multi_stage count the passes run by generated kernels and those among them of
two or more stages.  --plan-only plans the same circuits on the host and runs nothing (no GPU
needed).  Exit status 1 on any failure or missing class."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "cuda-quantum-simulator_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("QSIM_CACHE", "0")


def planned(fc, plan, qsim, s):
    """(circuits, classes, generated passes, multi-stage ones) as the host plans configuration s."""
    if s.get("jit"):
        infos = [info for _, _, info in fc.generated_circuits(qsim, s)]
    else:
        infos = [plan.plan_stage_info(fc.circuit_of(qsim, s["n"], gates)) for _, gates, _ in fc.cases(s)]
    hit, staged = set(), []
    for info in infos:
        hit |= fc.classes_of(info)
        staged += [p for p in info["passes"] if not p["single"] and p["rb"] > 0]
    jit = len(staged) if s.get("jit") else 0
    return len(infos), hit, jit, sum(p["stages"] >= 2 for p in staged) if jit else 0


def main(argv):
    import fused_cases as fc
    import qsim_amd
    from qsim_amd import plan

    plan_only = "--plan-only" in argv
    idx = [int(a) for a in argv if not a.startswith("--")]
    out = {"cases": 0, "worst": 0.0, "failures": [], "missing": [], "jit_passes": 0, "multi_stage": 0}
    if len(idx) != 1 or (not plan_only and qsim_amd.device_count() < 1):
        out["failures"] = ["no variant given or no GPU visible"]
        print(json.dumps(out))
        return 1
    for s in fc.CHILDREN[idx[0]]:
        fc.apply_settings(plan, s)
        plan.set_jit(2 if s.get("jit") else 0, 0 if s.get("jit") else -1)
        if plan_only:
            ran, hit, jp, multi = planned(fc, plan, qsim_amd, s)
            w, bad = 0.0, []
        elif s.get("jit"):
            ran, w, bad, hit, jp, multi = fc.run_generated(qsim_amd, s)
        else:
            ran, w, bad, hit = fc.run_matrix(qsim_amd, s)
            jp = multi = 0
        out["cases"] += ran
        out["worst"] = max(out["worst"], w)
        out["failures"] += bad
        out["missing"] += [repr(m) for m in fc.missing(fc.required(s), hit)]
        out["jit_passes"] += jp
        out["multi_stage"] += multi
        if bad:  # nothing more on the GPU after a failing size
            break
    print(json.dumps(out))
    return 1 if out["failures"] or out["missing"] else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
