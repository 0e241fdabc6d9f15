"""GPU: batch_multi_bev_gen <root> <sensor_type> <raw_format> — keyframe_point_cloud/ holds the selectors' INPUT (raw
.bin sweeps, read by host/RawSweeps.cpp and projected on the GPU) instead of their output.  The tool must then write,
file for file, what it writes for the PCDs the selectors' projection (the oracle's literal restatement) makes of the same
sweeps: .bin, .csv, non_ground_point_cloud/*.pcd and keyframe_label.csv."""
import os
import subprocess

import numpy as np
import pytest

import bev_amd
import oracle_lib as orc
import pcd_util
import rawsweeps_lib as rs
from projection_data import KITTI_VARIANTS, kitti_returns, raw_returns
from test_cli_gpu import CLI, _pose_line, _tree

pytestmark = pytest.mark.gpu
FORMAT = {rs.MULRAN: ("mulran", "OS1_64"), rs.OXFORD: ("oxford", "HDL_32E"), rs.KITTI: ("kitti", "HDL_64E")}


def _sweep_files(kind):
    """12 raw files as the dataset would hold them: one empty, one with a partial trailing record, for MulRan one above
    the selector's cap of 64 * 1024 returns"""
    if kind == rs.KITTI:
        sweeps = [kitti_returns(i, KITTI_VARIANTS[i % len(KITTI_VARIANTS)]) for i in range(11)]
    else:
        pool = raw_returns(70000, 21, nonfinite=False)
        top = 65536 if kind == rs.MULRAN else 36000
        sweeps = [np.roll(pool, 913 * i, axis=0)[:top - 2900 * i] for i in range(11)]
        if kind == rs.MULRAN:
            sweeps[4] = np.roll(pool, 5, axis=0)[:66000]          # 464 returns above the cap
    data = [(np.ascontiguousarray(s.T) if kind == rs.OXFORD else np.ascontiguousarray(s)).astype("<f4").tobytes() for s in sweeps]
    data[7] += b"\x00\x00\x80\x3f\x00\x00\x00\x40\x01"            # a partial trailing record (9 bytes)
    data.insert(2, b"")                                           # an empty file
    return data


@pytest.mark.parametrize("kind", [rs.MULRAN, rs.OXFORD, rs.KITTI])
def test_raw_tree_equals_the_projected_pcd_tree(tmp_path, kind):
    assert CLI.exists(), "host CLI not built"
    raw_format, sensor = FORMAT[kind]
    files = _sweep_files(kind)
    assert len(files) == 12
    a, b = tmp_path / "raw", tmp_path / "pcd"
    for root in (a, b):
        (root / "keyframe_point_cloud").mkdir(parents=True)
        (root / "keyframe_pose.csv").write_text(
            "\n".join(_pose_line(i, 9.0 * i, 0.7 * i, 0.0, 0.02 * i) for i in range(len(files))) + "\n")
    for i, data in enumerate(files):
        (a / "keyframe_point_cloud" / f"{i:06d}.bin").write_bytes(data)
        cloud = orc.project(kind, rs.expected(kind, data))        # the file as the reader defines it, projected
        pcd_util.write_pcd_binary(b / "keyframe_point_cloud" / f"{i:06d}.pcd", cloud)
    (a / "keyframe_point_cloud" / "000003.pcd").write_text("not listed in raw mode")
    env = dict(os.environ, BEV_NO_PNG="1", BEV_BATCH="5")
    ra = subprocess.run([str(CLI), str(a), sensor, raw_format], capture_output=True, text=True, timeout=600, env=env)
    rb = subprocess.run([str(CLI), str(b), sensor], capture_output=True, text=True, timeout=600, env=env)
    assert ra.returncode == 0 and rb.returncode == 0, ra.stdout[-2000:] + ra.stderr[-2000:] + rb.stderr[-2000:]
    names = [f"Converting file: {i:06d}" for i in range(len(files))]
    assert [l for l in ra.stdout.splitlines() if l.startswith("Converting file: ")] == names
    ta, tb = _tree(a), _tree(b)
    assert len(tb) == 3 * len(files) + 1 and ta.keys() == tb.keys(), sorted(set(ta) ^ set(tb))[:6]
    assert all(ta[k] == tb[k] for k in tb), [k for k in tb if ta[k] != tb[k]][:6]
    # ... and what both wrote is the oracle's hot path on the projected cloud (one frame looked at)
    sp = orc.sensor_from_params(bev_amd.params_for_sensor(sensor))
    o_ord, _, o_multi, _ = orc.process_frame(sp, orc.project(kind, rs.expected(kind, files[5])))
    assert ta["output_multi_bev/binary/000005.bin"] == o_multi.tobytes()
    _, cloud = pcd_util.read_pcd_binary(a / "non_ground_point_cloud" / "000005.pcd")
    assert cloud.tobytes() == o_ord.tobytes()


def test_a_raw_format_that_does_not_fit_the_sensor_touches_nothing(tmp_path):
    root = tmp_path / "kf"
    (root / "keyframe_point_cloud").mkdir(parents=True)
    (root / "keyframe_point_cloud" / "000000.bin").write_bytes(raw_returns(3000, 1).tobytes())
    (root / "output_multi_bev" / "binary").mkdir(parents=True)
    kept = root / "output_multi_bev" / "binary" / "earlier.bin"
    kept.write_text("an earlier run's output")
    for sensor, raw_format, words in [("HDL_32E", "kitti", "does not fit"), ("OS1_64", "oxford", "does not fit"),
                                      ("HDL_64E", "mulran", "does not fit"), ("OS1_64", "ouster", "unknown raw_format")]:
        r = subprocess.run([str(CLI), str(root), sensor, raw_format], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and words in r.stderr, (sensor, raw_format, r.stderr)
        assert kept.read_text() == "an earlier run's output"
        assert not (root / "non_ground_point_cloud").exists()
