"""GPU: batch_posed_bev_gen (host C++ over bev_posed_bev_batch) end to end: the labelled clouds of
non_ground_point_cloud/ under every pose of a pose file, BEV_BATCH files per call.  The output trees do not depend on the
batch size, an unreadable file in the middle of a batch goes on as an empty cloud, every .bin is the oracle's, every .csv has
the main tool's size and parses back to the oracle's single-layer image."""
import os
import subprocess

import numpy as np
import pytest

import bev_amd
import oracle_lib as orc
import pcd_util
from bev_amd import synth

pytestmark = pytest.mark.gpu
CLI = bev_amd.PKG_DIR / "host" / "batch_posed_bev_gen"
POSE_TEXT = "# tx ty tz yaw_deg\n1.5 -2.25 0.125 30\n\n  -3 4 1 -45.5\n0 0 0 0\n"
POSES = [(1.5, -2.25, 0.125, 30.0), (-3.0, 4.0, 1.0, -45.5), (0.0, 0.0, 0.0, 0.0)]


def _tree(root):
    return {str(f.relative_to(root)): f.read_bytes() for f in sorted((root / "output_posed_bev").rglob("*")) if f.is_file()}


def test_batches_give_the_same_tree_and_the_oracles_images(tmp_path):
    assert CLI.exists(), "host CLI not built"
    p = bev_amd.params_for_sensor("HDL_64E")
    sp = orc.sensor_from_params(p)
    marked = orc.mark_ground(sp, orc.order_cloud(sp, synth.sweep(p, 3)))[0]
    empty = np.empty(0, bev_amd.POINT_DTYPE)
    frames = {"000000": marked[:30000], "000001": synth.adversarial(p, 5000, 9, nonfinite=True),
              "000002": None,   # unreadable: the last file of the first batch of two, the middle of the batch of five
              "000003": marked[60000:60257], "000004": empty}
    poses = tmp_path / "poses.txt"
    poses.write_text(POSE_TEXT)
    runs = {}
    for batch in (2, 5):
        root = tmp_path / f"kf{batch}"
        (root / "non_ground_point_cloud").mkdir(parents=True)
        for name, pts in frames.items():
            path = root / "non_ground_point_cloud" / f"{name}.pcd"
            if pts is None:
                path.write_bytes(b"not a point cloud\n" * 7)
            else:
                pcd_util.write_pcd_binary(path, pts)
        (root / "output_posed_bev" / "binary").mkdir(parents=True)
        (root / "output_posed_bev" / "binary" / "stale.bin").write_text("must be removed")
        env = dict(os.environ, BEV_BATCH=str(batch), BEV_MAX_POINTS=str(p.slots))
        r = subprocess.run([str(CLI), str(root), "HDL_64E", str(poses)], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        assert [l for l in r.stdout.splitlines() if l.startswith("Converting file: ")] == [f"Converting file: {n}" for n in frames]
        assert r.stdout.rstrip().endswith("Done.")
        assert r.stderr.count("Can not read") == 1 and "000002.pcd" in r.stderr
        runs[batch] = _tree(root)

    assert sorted(runs[2]) == sorted(f"output_posed_bev/{d}/{n}_{k:02d}.{e}" for n in frames for k in range(3)
                                     for d, e in (("binary", "bin"), ("csv", "csv")))
    assert runs[2] == runs[5]

    for name, pts in frames.items():
        cloud = empty if pts is None else pts
        for k, pose in enumerate(POSES):
            moved = orc.transform_cloud(cloud, orc.yaw_translate_matrix(*pose))
            want_multi, want_single = orc.multi_bev(sp, moved, 1.0), orc.single_bev(moved, 1.0)
            b = runs[2][f"output_posed_bev/binary/{name}_{k:02d}.bin"]
            assert len(b) == 1204224 and b == want_multi.tobytes(), (name, k)
            csv = runs[2][f"output_posed_bev/csv/{name}_{k:02d}.csv"].decode()
            assert len(csv) == 250656, (name, k)
            assert np.array_equal(np.array([[int(v) for v in l.split(",")] for l in csv.splitlines()], np.uint8), want_single), (name, k)
    assert any(runs[2][f"output_posed_bev/binary/000000_{k:02d}.bin"].count(b"\xff") for k in range(3))
