"""GPU: batch_submap_cloud_manip (host C++ over bev_submap_float_bev_batch) end to end, from a tree written by
batch_cloud_manip on a few short synthetic finite sweeps.  A half window of 0 reproduces that tool's own output_bvm CSVs and
PNGs; windows of 5 frames at stride 3 under axis-aligned relative poses equal the oracle's composition through the same CSV
formatter, whatever BEV_BATCH is."""
import os
import subprocess

import numpy as np
import pytest

import bev_amd
import oracle_lib as orc
import pcd_util
from bev_amd import synth
from test_cli_manip_gpu import _csv_text, _png_of
from test_cli_submap_gpu import N, _pose_line, _relative

pytestmark = pytest.mark.gpu
MANIP = bev_amd.PKG_DIR / "host" / "batch_cloud_manip"
CLI = bev_amd.PKG_DIR / "host" / "batch_submap_cloud_manip"
SIZES = [20000, 257, 70000, 1025, 0, 33000, 4097, 12000]


def _tree(root):
    return {str(f.relative_to(root)): f.read_bytes() for f in sorted((root / "output_submap_bvm").rglob("*")) if f.is_file()}


def test_windows_of_a_tree_batch_cloud_manip_wrote(tmp_path):
    assert MANIP.exists() and CLI.exists(), "host CLIs not built"
    p = bev_amd.params_for_sensor("HDL_64E")
    root = tmp_path / "kf"
    (root / "keyframe_point_cloud").mkdir(parents=True)
    names = [f"{i:06d}" for i in range(N)]
    assert len(SIZES) == N
    for i, name in enumerate(names):
        sweep = synth.sweep(p, 40 + i)[:SIZES[i]]
        assert np.isfinite(sweep["x"]).all() and np.isfinite(sweep["y"]).all() and np.isfinite(sweep["z"]).all()
        pcd_util.write_pcd_binary(root / "keyframe_point_cloud" / f"{name}.pcd", sweep)
    (root / "keyframe_pose.csv").write_text("\n".join(_pose_line(i) for i in range(N)) + "\n")
    env = dict(os.environ, BEV_MAX_POINTS=str(p.slots))
    r = subprocess.run([str(MANIP), str(root)], capture_output=True, text=True, timeout=300, env=env)   # writes non_ground_point_cloud/
    assert r.returncode == 0, r.stdout + r.stderr

    # half window 0: every map is its key frame under the identity
    (root / "output_submap_bvm").mkdir()
    (root / "output_submap_bvm" / "stale.csv").write_text("must be removed")
    r = subprocess.run([str(CLI), str(root), "HDL_64E", "0"], capture_output=True, text=True, timeout=300, env=dict(env, BEV_BATCH="3"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert [l for l in r.stdout.splitlines() if l.startswith("Converting file: ")] == [f"Converting file: {n}" for n in names]
    assert r.stdout.rstrip().endswith("Done.")
    own = _tree(root)
    assert sorted(own) == sorted(f"output_submap_bvm/{n}.{e}" for n in names for e in ("csv", "png"))
    for name in names:
        for e in ("csv", "png"):
            assert own[f"output_submap_bvm/{name}.{e}"] == (root / "output_bvm" / f"{name}.{e}").read_bytes(), (name, e)
    assert any(c not in b"0, \n" for c in own[f"output_submap_bvm/{names[0]}.csv"])      # not an empty grid

    # half window 2, stride 3: keys 0, 3, 6
    clouds = [pcd_util.read_pcd_binary(root / "non_ground_point_cloud" / f"{n}.pcd")[1] for n in names]
    runs = {}
    for batch in (2, 5):
        r = subprocess.run([str(CLI), str(root), "HDL_64E", "2", "3"], capture_output=True, text=True, timeout=300,
                           env=dict(env, BEV_BATCH=str(batch)))
        assert r.returncode == 0, r.stdout + r.stderr
        runs[batch] = _tree(root)
    keys = [0, 3, 6]
    assert sorted(runs[2]) == sorted(f"output_submap_bvm/{names[i]}.{e}" for i in keys for e in ("csv", "png"))
    assert runs[2] == runs[5]
    for i in keys:
        moved = [orc.transform_cloud(clouds[j], np.eye(3, 4, dtype=np.float32).reshape(12) if j == i else _relative(i, j))
                 for j in range(max(0, i - 2), min(N - 1, i + 2) + 1)]
        want = orc.float_bev(np.concatenate(moved), 1.0, True)
        assert want.shape == (201, 201)
        assert runs[2][f"output_submap_bvm/{names[i]}.csv"].decode() == _csv_text(want), i
        assert np.array_equal(pcd_util.read_png_gray8(root / "output_submap_bvm" / f"{names[i]}.png"), _png_of(want)), i
        assert runs[2][f"output_submap_bvm/{names[i]}.csv"] != (root / "output_bvm" / f"{names[i]}.csv").read_bytes()   # more than the key frame alone
