"""The reference's own ``code_single/tools/eval_lidar.py`` (chamfer distance and range RMSE of the rendered against the measured
LiDAR sweep), source unchanged, on an experiment its trainer wrote on this package."""
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import ref_glue

ROOT = Path(__file__).resolve().parent.parent
TOOL = Path("/root/reference") / "code_single/tools/eval_lidar.py"
needs_reference = ref_glue.needs_reference(ref_glue.readable(TOOL), reason="executes the reference's own sources, which only the authoring machine has (emulator backend)")
HEADER = ("cham_pred, cham_gt, chamfer, cham_pred_99, cham_gt_99, chamfer_99, cham_pred_97, cham_gt_97, chamfer_97, "
          "cham_pred_95, cham_gt_95, chamfer_95, depth, depth_99, depth_97, depth_95")
N_FRAMES = 6            # STREET_SMALL: --dataset_cfg.param.n_frames=6


@needs_reference
def test_reference_eval_lidar_tool_runs_unchanged(backend, tmp_path):
    """Train the StreetSurf config (``withmask_withlidar_joint.240219.yaml``) for 8 iterations with the ``STREET_SMALL`` overrides,
    then ``run_reference_train.py --script code_single/tools/eval_lidar.py --resume_dir <exp> --lidar_id lidar_TOP``: return code
    0; ``chamfer_dis_and_depth_err.txt`` has the tool's header and one row of 16 finite, non-negative numbers per frame whose
    ``chamfer*`` columns are the sums of their two terms to the printed precision; ``*_misc.json`` has
    ``chamfer == chamfer_pred + chamfer_gt`` and ``chamfer_95 <= chamfer_97 <= chamfer_99 <= chamfer`` (and the same for the
    range error).  An 8-iteration model renders a poor sweep: no quality threshold.

    Not checked: the first frame's ``cham_pred`` / ``cham_gt`` against ``pointcloud.chamfer_distance`` on clouds rebuilt in the
    test.  Rebuilding them means repeating the tool's own scene, asset-bank, data-loader and renderer set-up and its LiDAR
    filters in the test, i.e. a second copy of the tool; the operator itself is pinned bit for bit by tests/test_pointcloud.py,
    and the tool calls it through ``nr3d_lib.maths`` (asserted there to be the same function)."""
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    from test_reference_train import STREET_CFG, STREET_SMALL
    exp = tmp_path / "street"
    env = dict(os.environ, PYTHONWARNINGS="ignore")
    launcher = [sys.executable, str(ROOT / "tools" / "run_reference_train.py"), "--emulate"]
    r = subprocess.run(launcher + ["--config", str(STREET_CFG), "--exp_dir", str(exp), "--num_iters=8", "--training.i_val=-1"]
                       + STREET_SMALL, capture_output=True, text=True, timeout=1500, env=env, cwd=str(ROOT))
    assert r.returncode == 0 and "Everything done." in r.stdout, (r.stdout + r.stderr)[-3000:]
    rr = subprocess.run(launcher + ["--script", "code_single/tools/eval_lidar.py", "--resume_dir", str(exp), "--lidar_id",
                                    "lidar_TOP", "--dirname", "eval_lidar", "--rayschunk", "512", "--outbase", "t"],
                        capture_output=True, text=True, timeout=1500, env=env, cwd=str(ROOT))
    assert rr.returncode == 0, (rr.stdout + rr.stderr)[-3000:]
    out = exp / "eval_lidar"
    lines = (out / "chamfer_dis_and_depth_err.txt").read_text().strip().splitlines()
    assert lines[0] == HEADER
    assert len(lines) == 1 + N_FRAMES, lines
    for line in lines[1:]:
        v = [float(s) for s in line.split(",")]
        assert len(v) == 16 and all(math.isfinite(a) and a >= 0 for a in v), line
        for q in range(0, 12, 3):           # five printed decimals: each term is off by at most 5e-6
            assert abs(v[q + 2] - (v[q] + v[q + 1])) <= 1.6e-5, line
    misc_files = list(out.glob("*_misc.json"))
    assert len(misc_files) == 1, list(out.iterdir())
    m = json.loads(misc_files[0].read_text())
    for tag in ("", "_99", "_97", "_95"):
        for k in ("chamfer_pred", "chamfer_gt", "chamfer", "depth_error"):
            assert math.isfinite(m[k + tag]) and m[k + tag] >= 0, (k + tag, m)
        assert abs(m["chamfer" + tag] - (m["chamfer_pred" + tag] + m["chamfer_gt" + tag])) <= 1e-9 * max(1.0, m["chamfer" + tag])
    assert m["chamfer_95"] <= m["chamfer_97"] <= m["chamfer_99"] <= m["chamfer"]
    assert m["depth_error_95"] <= m["depth_error_97"] <= m["depth_error_99"] <= m["depth_error"]
