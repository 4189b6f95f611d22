#!/usr/bin/env python3
"""Per-pair errors of vt_collision_loss against the float64 model (tests/collide_model.py) on the families of tests/collide_cases.py, as fractions of the gates of
tests/test_gpu_collide.py, with the float32 oracle's E32 measured afresh next to the recorded figures.  Measurements only: the gates are derived in the test and are
not tuned to this report.  Needs the GPU.  Usage: tools/collide_perpair_report.py [out.txt]  (profiles/r20_collide_perpair.txt is its output)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import collide_cases as C  # noqa: E402


def main():
    lines = ["# worst |kernel - model| / gate per family; gates: value 8 E32_V u S_V + n_f 2^-41, gradient (8 E32_g u S_g + n_f 2^-41) gscale / B + u |dt64|, u = 2^-24;",
             "# pair counts are compared exactly on every frame without an undecided pair (|margin| < 64 u max|coordinate|).",
             "# counts: frames with a wrong pair count, plus frames without pairs that moved an output and frames that alone differ from the frame in their batch.",
             "# fit_like: each frame against the nearest resolution of its undecided pairs.",
             "%-9s %6s %7s %9s %9s %8s %7s  %-15s %-15s  %7s %8s %8s" % ("family", "calls", "frames", "colliding", "undecided", "left out", "counts", "E32 recorded", "E32 measured",
                                                                          "value", "gradient", "term")]
    for fam, cases in C.FAMILY.items():
        eV = eg = 0.0; w = dict(pairs=0, value=0.0, grad=0.0, term=0.0, left_out=0); frames = coll = und = 0
        for name, mc in cases:
            a, b, _ = C.measure_e32(name, mc); eV, eg = max(eV, a), max(eg, b)
            ref = C.reference(name, mc); frames += len(ref); coll += sum(r["pairs"] > 0 for r in ref); und += sum(bool(r["undecided"].any()) for r in ref)
            if fam == "fit_like":                            # compared with the nearest resolution of its undecided pairs (no frame left out)
                fr, term = C.measure_fit_like()
                w = dict(pairs=sum(not f["matched"] for f in fr), value=max(f["value"] for f in fr), grad=max(f["grad"] for f in fr), term=term, left_out=0)
                bad = sum(f["differ"] or not f["in_slack"] for f in fr)
            else:
                o = C.measure_case(name, mc); bad = o["moved"] + o["differ"]
                w = dict(pairs=w["pairs"] + o["pairs"], value=max(w["value"], o["value"]), grad=max(w["grad"], o["grad"]), term=max(w["term"], o["term"]), left_out=w["left_out"] + o["left_out"])
            w["pairs"] += bad                                # a frame that moved without pairs or differs from its batch counts as a wrong frame
        over = w["pairs"] > 0 or max(w["value"], w["grad"], w["term"]) > 1
        lines.append("%-9s %6d %7d %9d %9d %8d %7d  %-15s %-15s  %7.3f %8.3f %8.3f%s" % (fam, len(cases), frames, coll, und, w["left_out"], w["pairs"], "%.3f %.3f" % C.E32[fam], "%.4f %.4f" % (eV, eg),
                                                                                   w["value"], w["grad"], w["term"], "   EXCEEDS A GATE" if over else ""))
    text = "\n".join(lines) + "\n"
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as fh:
            fh.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
