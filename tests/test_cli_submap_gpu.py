"""GPU: batch_submap_bev_gen (host C++ over bev_submap_bev_batch) end to end, from a tree written by
batch_multi_bev_gen on synthetic finite sweeps.  A half window of 0 reproduces that tool's own images; windows of 5 frames at
stride 3 under axis-aligned relative poses equal the oracle's composition, whatever BEV_BATCH is."""
import os
import subprocess

import numpy as np
import pytest

import bev_amd
import oracle_lib as orc
import pcd_util
from bev_amd import synth

pytestmark = pytest.mark.gpu
MAIN = bev_amd.PKG_DIR / "host" / "batch_multi_bev_gen"
CLI = bev_amd.PKG_DIR / "host" / "batch_submap_bev_gen"
N = 8

# Rotations about x, y and z by multiples of 90 degrees (entries 0 / +-1) and translations in multiples of 0.25 m: every product
# and sum of R_i^T R_j and R_i^T (t_j - t_i) is exact in double, so numpy gives the tool's matrices whatever the order of
# evaluation (up to the sign of a zero, which does not reach the images).
RZ = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float64)
RX = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], np.float64)
RY = np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], np.float64)
ROT = [np.eye(3), RZ, RZ @ RZ, RX, RZ @ RZ @ RZ, RY, RX @ RZ, np.eye(3)]
TRANS = np.array([[0, 0, 0], [2.25, 0.5, 0], [4.0, -1.25, 0.25], [6.5, 0, 0.5], [8.0, 3.75, 0], [10.25, 4.0, -0.25], [12.0, 2.5, 0],
                  [13.75, 0.25, 0.25]], np.float64)


def _pose_line(i):
    return ",".join([str(i)] + [repr(float(v)) for v in TRANS[i]] + ["0", "0", "0"] + [repr(float(v)) for v in ROT[i].reshape(9)])


def _relative(i, j):
    m = np.zeros((3, 4), np.float64)
    m[:, :3] = ROT[i].T @ ROT[j]
    m[:, 3] = ROT[i].T @ (TRANS[j] - TRANS[i])
    return m.astype(np.float32).reshape(12)


def _tree(root):
    return {str(f.relative_to(root)): f.read_bytes() for f in sorted((root / "output_submap_bev").rglob("*")) if f.is_file()}


def test_windows_of_a_tree_the_main_tool_wrote(tmp_path):
    assert MAIN.exists() and CLI.exists(), "host CLIs not built"
    p = bev_amd.params_for_sensor("HDL_32E")
    sp = orc.sensor_from_params(p)
    root = tmp_path / "kf"
    (root / "keyframe_point_cloud").mkdir(parents=True)
    names = [f"{i:06d}" for i in range(N)]
    for i, name in enumerate(names):
        sweep = synth.sweep(p, 40 + i, keep=0.6)
        assert np.isfinite(sweep["x"]).all() and np.isfinite(sweep["y"]).all() and np.isfinite(sweep["z"]).all()
        pcd_util.write_pcd_binary(root / "keyframe_point_cloud" / f"{name}.pcd", sweep)
    (root / "keyframe_pose.csv").write_text("\n".join(_pose_line(i) for i in range(N)) + "\n")
    env = dict(os.environ, BEV_NO_PNG="1", BEV_MAX_POINTS=str(p.slots))
    r = subprocess.run([str(MAIN), str(root), "HDL_32E"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr

    # half window 0: every map is its key frame under the identity
    (root / "output_submap_bev" / "binary").mkdir(parents=True)
    (root / "output_submap_bev" / "binary" / "stale.bin").write_text("must be removed")
    r = subprocess.run([str(CLI), str(root), "HDL_32E", "0"], capture_output=True, text=True, timeout=300, env=dict(env, BEV_BATCH="3"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert [l for l in r.stdout.splitlines() if l.startswith("Converting file: ")] == [f"Converting file: {n}" for n in names]
    assert r.stdout.rstrip().endswith("Done.")
    own = _tree(root)
    assert sorted(own) == sorted(f"output_submap_bev/{d}/{n}.{e}" for n in names for d, e in (("binary", "bin"), ("csv", "csv")))
    for name in names:
        assert own[f"output_submap_bev/binary/{name}.bin"] == (root / "output_multi_bev" / "binary" / f"{name}.bin").read_bytes(), name
        assert own[f"output_submap_bev/csv/{name}.csv"] == (root / "output_single_bev" / "csv" / f"{name}.csv").read_bytes(), name
    assert own[f"output_submap_bev/binary/{names[0]}.bin"].count(b"\xff")

    # half window 2, stride 3: keys 0, 3, 6
    clouds = [pcd_util.read_pcd_binary(root / "non_ground_point_cloud" / f"{n}.pcd")[1] for n in names]
    runs = {}
    for batch in (2, 5):
        r = subprocess.run([str(CLI), str(root), "HDL_32E", "2", "3"], capture_output=True, text=True, timeout=300,
                           env=dict(env, BEV_BATCH=str(batch)))
        assert r.returncode == 0, r.stdout + r.stderr
        runs[batch] = _tree(root)
    keys = [0, 3, 6]
    assert sorted(runs[2]) == sorted(f"output_submap_bev/{d}/{names[i]}.{e}" for i in keys for d, e in (("binary", "bin"), ("csv", "csv")))
    assert runs[2] == runs[5]
    for i in keys:
        moved = [orc.transform_cloud(clouds[j], np.eye(3, 4, dtype=np.float32).reshape(12) if j == i else _relative(i, j))
                 for j in range(max(0, i - 2), min(N - 1, i + 2) + 1)]
        cloud = np.concatenate(moved)
        want_multi, want_single = orc.multi_bev(sp, cloud, 1.0), orc.single_bev(cloud, 1.0)
        b = runs[2][f"output_submap_bev/binary/{names[i]}.bin"]
        assert len(b) == 1204224 and b == want_multi.tobytes(), i
        csv = runs[2][f"output_submap_bev/csv/{names[i]}.csv"].decode()
        assert len(csv) == 250656, i
        assert np.array_equal(np.array([[int(v) for v in l.split(",")] for l in csv.splitlines()], np.uint8), want_single), i
        assert b != (root / "output_multi_bev" / "binary" / f"{names[i]}.bin").read_bytes()   # more than the key frame alone
