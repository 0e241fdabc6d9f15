"""GPU: batch_cloud_manip in batches (BEV_BATCH files per bev_process_batch + bev_float_bev_batch call): the
output trees do not depend on the batch size and are the oracle's, an unreadable file in the middle of a batch goes on as
an empty cloud, and stdout keeps one pair of lines per file, in file order."""
import os
import subprocess

import numpy as np
import pytest

import bev_amd
import oracle_lib as orc
import pcd_util
from bev_amd import synth
from test_cli_manip_gpu import _csv_text, _png_of

pytestmark = pytest.mark.gpu
BATCH_CLI = bev_amd.PKG_DIR / "host" / "batch_cloud_manip"


def _tree(root):
    return {str(f.relative_to(root)): f.read_bytes() for d in ("output_bvm", "non_ground_point_cloud")
            for f in sorted((root / d).rglob("*")) if f.is_file()}


def test_batches_give_the_trees_of_single_files(tmp_path):
    assert BATCH_CLI.exists(), "host CLI not built"
    p = bev_amd.params_for_sensor("HDL_64E")
    sp = orc.sensor_from_params(p)
    empty = np.empty(0, bev_amd.POINT_DTYPE)
    frames = {"000000": synth.sweep(p, 0), "000001": synth.adversarial(p, 20000, 9), "000002": empty,
              "000003": synth.sweep(p, 1)[:70000], "000004": synth.adversarial(p, 3000, 2),
              "000005": None,   # unreadable, second file of the second batch
              "000006": synth.sweep(p, 2), "000007": synth.sweep(p, 3)[:257], "000008": synth.adversarial(p, 50000, 5)}
    runs = {}
    for batch in (4, 1):
        root = tmp_path / f"kf{batch}"
        (root / "keyframe_point_cloud").mkdir(parents=True)
        for name, pts in frames.items():
            path = root / "keyframe_point_cloud" / f"{name}.pcd"
            if pts is None:
                path.write_bytes(b"not a point cloud\n" * 7)
            else:
                pcd_util.write_pcd_binary(path, pts)
        env = dict(os.environ, BEV_BATCH=str(batch), BEV_MAX_POINTS=str(p.slots + 8192))
        r = subprocess.run([str(BATCH_CLI), str(root)], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = [l for l in r.stdout.splitlines() if l.startswith(("Converting file: ", "[TIME] Preprocessing and BEV generation: "))]
        assert len(lines) == 2 * len(frames)
        assert lines[0::2] == [f"Converting file: {n}" for n in frames]
        assert all(l.startswith("[TIME] Preprocessing") and l.endswith("ms. ") for l in lines[1::2])
        assert "[TIME] Average preprocessing and BEV generation: " in r.stdout and r.stdout.rstrip().endswith("Done.")
        assert r.stderr.count("Can not read") == 1 and "000005.pcd" in r.stderr
        runs[batch] = _tree(root)

    assert sorted(runs[4]) == sorted([f"output_bvm/{n}.{e}" for n in frames for e in ("csv", "png")] +
                                     [f"non_ground_point_cloud/{n}.pcd" for n in frames])
    assert runs[4] == runs[1]

    root = tmp_path / "kf4"
    for name, pts in frames.items():
        ordered, _, _ = orc.mark_ground(sp, orc.order_cloud(sp, empty if pts is None else pts))
        want = orc.float_bev(ordered, 1.0, True)               # label == 0 skipped (:218)
        assert want.shape == (201, 201)
        assert (root / "output_bvm" / f"{name}.csv").read_text() == _csv_text(want)
        assert np.array_equal(pcd_util.read_png_gray8(root / "output_bvm" / f"{name}.png"), _png_of(want))
        head, cloud = pcd_util.read_pcd_binary(root / "non_ground_point_cloud" / f"{name}.pcd")
        assert f"POINTS {p.slots}" in head
        assert cloud.tobytes() == ordered.tobytes()
