"""GPU (-m gpu): the plain bench.py run (the headline line only, everything else behind --full) and --dump-outputs (what the last timed step
returned), checked against the fitted rows bench.py already writes for the whole job (VT_BENCH_DUMP_ROWS)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def test_plain_bench_line_and_dump_outputs(tmp_path):
    out_dir = tmp_path / "out"
    # 2 batches of a 250-frame sequence (frames 0-96 and 96-192) at 1/8 map resolution, one stream
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "0", "--streams", "1", "--sequence", "250",
           "--res-scale", "0.125", "--dump-outputs", str(out_dir)]
    env = dict(os.environ, VT_BENCH_WATCHDOG="600", VT_BENCH_DUMP_ROWS=str(tmp_path / "rows.npy"))
    out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900, cwd=ROOT)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode == 0 and len(lines) == 1, out.stdout[-2000:] + out.stderr[-4000:]
    line = json.loads(lines[0])
    assert line["metric"] == "frames/sec joint SMPL+object fit" and line["unit"] == "frames/s" and line["higher_is_better"] is True and line["dtype"]
    assert line["steps"] == 2 and line["config"]["frames_timed"] == 192
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 * 2 - 192) < 1e-6 * 192
    # a plain run measures the headline only: no informational leg, no CPU baseline, no solo-kernel figures
    for k in ("full_schedule", "smplt_prefit", "strict_fp32", "sifnet_inference", "demo_pipeline", "cpu_baseline", "dynamic_handout"):
        assert k not in line, k
    assert line["roofline"]["solo_launch_ms"] is None and line["roofline"]["launches"] > 0
    # the dump is the last timed step (job 1 = frames 96-192): its parameters are that batch's fitted rows, bit for bit
    names = ("pose", "betas", "trans", "obj_R", "obj_t", "obj_s", "smpl_stage_losses", "object_stage_losses")
    assert sorted(os.listdir(out_dir)) == sorted(n + ".npy" for n in names)
    d = {n: np.load(out_dir / (n + ".npy")) for n in names}
    assert all(d[n].dtype == np.float32 for n in names[:6]) and all(d[n].dtype == np.float64 for n in names[6:])
    rows = np.load(tmp_path / "rows.npy")
    mine = np.concatenate([d["pose"], d["betas"], d["trans"], d["obj_R"].reshape(-1, 9), d["obj_t"], d["obj_s"][:, None]], 1)
    assert rows.shape == (192, 182) and np.array_equal(mine, rows[96:192])
    for n in names[6:]:
        assert len(d[n]) > 0 and np.isfinite(d[n]).all(), n
