#!/usr/bin/env python3
"""Record what tests/test_gpu_encoder_kernels.py measured: runs the file with -s on the GPU (or reads a kept output with --from-log) and writes, per case, the worst
channel and its fraction of the per-channel gate, the worst fraction of the element backstop, and the statistics' fractions at each mean / std ratio to
profiles/r18_encoder_perchannel.txt.  The report records; the gates are not tuned to it."""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(); ap.add_argument("--from-log"); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_encoder_perchannel.txt"))
    a = ap.parse_args()
    if a.from_log:
        text = open(a.from_log).read()
    else:
        text = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_encoder_kernels.py"), "-m", "gpu", "-q", "-s", "--durations=5",
                               "-p", "no:cacheprovider"], cwd=ROOT, capture_output=True, text=True).stdout
    keep = [ln.lstrip(".").rstrip() for ln in text.splitlines() if re.search(r"of (its gate|the backstop)|passed|failed|^\d+\.\d+s call", ln.lstrip("."))]
    worst = {}
    for ln in keep:
        for kind, pat in (("channel gate", r"at ([\d.]+) of its gate \(err"), ("element backstop", r"worst element ([\d.]+) of the backstop"), ("stem / up-sampling / GroupNorm apply element gate",r"worst element ([\d.]+) of its gate"),
                          ("statistics: mean", r"mean ([\d.]+) of its gate"), ("statistics: rstd", r"rstd ([\d.]+) of its gate")):
            m = re.search(pat, ln)
            if m and float(m.group(1)) >= worst.get(kind, (-1, ""))[0]:
                worst[kind] = (float(m.group(1)), ln)
    with open(a.out, "w") as f:
        f.write("tests/test_gpu_encoder_kernels.py on one MI355X: fractions of the gates (1 = at the gate)\n\nworst of each kind:\n")
        for kind, (v, ln) in worst.items():
            f.write("  %-52s %.3f   %s\n" % (kind, v, ln.split(":")[0]))
        f.write("\nevery case:\n" + "\n".join(keep) + "\n")
    print("wrote", a.out, len(keep), "lines")


if __name__ == "__main__":
    main()
