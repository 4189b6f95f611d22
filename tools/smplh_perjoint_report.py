#!/usr/bin/env python3
"""Per-row errors of the SMPL-H kernels against the float64 model (tests/smplh_model.py) on the cases of tests/test_gpu_smplh_perjoint.py, next to the float32
CPU oracle's on the same inputs.  Needs the GPU.  Usage: tools/smplh_perjoint_report.py [out.txt]  (profiles/r14_smplh_perjoint.txt is its output)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import smplh_cases as C  # noqa: E402
import smplh_model as M  # noqa: E402
from vistracker_amd import synthetic as syn  # noqa: E402


def main():
    base = syn.smplh_model(0)
    lines = ["# worst per-row error (max |x - model| over the row / max |model| over the row) against the float64 model, kernel | float32 CPU oracle",
             "# rows: 52 joints of dpose, 10 columns of dbetas, 3 axes of dtrans; gate = %g x the oracle's worst row of the case; fwd = max |kernel - model| in m" % M.GATE,
             "%-12s %-5s %3s  %-19s %-19s %-19s %9s %9s  %s" % ("case", "djtr", "B", "dpose k | o32", "dbetas k | o32", "dtrans k | o32", "gate", "fwd", "worst joint")]
    for name in C.CASES:
        r = C.reference(name, base); c = r["inputs"]
        for mode in c["modes"]:
            fwd, grads = C.run_kernels(C.handle_of(name, c["model"]), c, mode)
            e = M.grad_errs(grads, r[mode]["ref"], c["zero_joints"]); o = r[mode]["err32"]
            f = max(float(np.abs(a - b).max()) for a, b in zip(fwd, r["fwd"]))
            cols = " ".join("%8.2e | %8.2e" % (e[k].max(), o[k].max()) for k in ("dpose", "dbetas", "dtrans"))
            lines.append("%-12s %-5s %3d  %s %9.2e %9.2e  %d%s" % (name, mode, len(c["pose"]), cols, r[mode]["gate"], f, int(e["dpose"].argmax()),
                                                                 "" if M.worst(e) <= r[mode]["gate"] else "   EXCEEDS THE GATE"))
    text = "\n".join(lines) + "\n"
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as fh:
            fh.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
