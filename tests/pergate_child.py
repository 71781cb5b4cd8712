"""Child process of tests/test_pergate_matrix_gpu.py: the per-gate operand matrix under one set of
launch-shape knobs (the QSIM_* variables gates.hip's Tune reads once per process, so every variant
needs a process of its own; the parent sets them in this process's environment).

    python tests/pergate_child.py 7 10 16

runs pergate_cases.run_matrix at each listed qubit count and prints one JSON line
{"cases": N, "worst": x, "failures": [...]}; exit status 1 on any failure."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "cuda-quantum-simulator_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("QSIM_CACHE", "0")


def main(argv):
    import pergate_cases as pc
    import qsim_amd

    sizes = [int(a) for a in argv]
    if not sizes or qsim_amd.device_count() < 1:
        print(json.dumps({"cases": 0, "worst": 0.0, "failures": ["no sizes given or no GPU visible"]}))
        return 1
    cases, worst, failures = 0, 0.0, []
    for n in sizes:
        ran, w, bad = pc.run_matrix(qsim_amd, n)
        cases += ran
        worst = max(worst, w)
        failures += bad
        if bad:  # nothing more on the GPU after a failing size
            break
    print(json.dumps({"cases": cases, "worst": worst, "failures": failures}))
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
