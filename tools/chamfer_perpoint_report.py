#!/usr/bin/env python3
"""Per-row errors of the contact Chamfer kernels against the float64 model (tests/chamfer_model.py) on the cases of tests/test_gpu_chamfer.py, as fractions of the
derived gates, and the per-point error of vt_nn_distance.  Measurements only: the gates are derived in tests/test_gpu_chamfer.py and are not tuned to this report.
Needs the GPU.  Usage: tools/chamfer_perpoint_report.py [out.txt]  (profiles/r16_chamfer_perpoint.txt is its output)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import chamfer_cases as C  # noqa: E402
import chamfer_model as M  # noqa: E402


def _fraction(g, want, gate):
    err = np.abs(g.astype(np.float64) - want)
    f = np.where(gate > 0, err / np.where(gate > 0, gate, 1), np.where(err > 0, np.inf, 0.0))
    return float(f.max()), int(f.max(1).argmax())


def main():
    lines = ["# worst gradient row: |g - model| / gate, gate = (n + 8) u S per row and component (start values: (n + 9) u (S + |start|)), u = 2^-24; n = terms added into",
             "# the row, S = sum of their absolute values, both from the float64 model.  term: |term - model| in units of u x term (gate 8).  '-': the form has no x gradient.",
             "%-24s %-8s %8s %5s  %9s %-16s %-16s" % ("case", "form", "gscale", "P", "term / u", "dx worst (row)", "dy worst (row)")]
    runs = [(n, None, False) for n in C.CASES] + [("edges", 900.0, False), ("edges", 2.0 ** -10, False), ("edges", None, True), ("many_pairs_1030", None, True)]
    for name, gscale, accumulate in runs:
        r = C.reference(name, gscale); x, y, offx, _ = C.packed(name); init = None
        if accumulate:
            rng = np.random.default_rng(5); init = tuple(rng.normal(0, 1e-3, a.shape).astype(np.float32) for a in (x, y))
        for form in C.FORMS:
            out = C.run_kernels(form, name, gscale=gscale, init=init)
            cols = []
            for k, i in (("x", 0), ("y", 1)):
                if out["d" + k] is None:
                    cols.append("-"); continue
                start = None if init is None else init[i]
                want = r["d" + k] if start is None else r["d" + k] + start.astype(np.float64)
                f, row = _fraction(out["d" + k], want, M.row_gate(r["n_" + k], r["S_" + k], start))
                cols.append("%.3f (%d)" % (f, row))
            te = abs(out["term"] - r["term"]) / (M.U * r["term"])
            bad = te > 8 or any(c != "-" and float(c.split()[0]) > 1 for c in cols)
            lines.append("%-24s %-8s %8g %5d  %9.3f %-16s %-16s%s" % (name + (" +start" if accumulate else ""), form, C.case(name)["gscale"] if gscale is None else gscale,
                                                                      len(offx) - 1, te, cols[0], cols[1], "   EXCEEDS A GATE" if bad else ""))
    worst = 0.0
    for nq, ns in C.NN_CASES:
        q, s = C.nn_case(nq, ns); want = M.nn_distance(q, s); d = C.run_nn(nq, ns).astype(np.float64)
        worst = max(worst, float((np.abs(d - want)[want > 0] / (M.U * want[want > 0])).max()))
    lines.append("vt_nn_distance, %d (nq, ns) shapes x 3 pairs: worst |d - model| = %.3f u x d (gate 4)" % (len(C.NN_CASES), worst))
    text = "\n".join(lines) + "\n"
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as fh:
            fh.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
