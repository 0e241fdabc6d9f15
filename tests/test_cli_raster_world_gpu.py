"""GPU: batch_submap_bev_gen, batch_submap_cloud_manip and batch_posed_bev_gen on the world of raster_world_cases.py
(DESIGN.md §6x), written as a tree of PCD files under non_ground_point_cloud/ (what the three tools read) and a
keyframe_pose.csv whose rows hold the poses' float32 entries, neither quarter turns nor multiples of 0.25 m.  What the tools
write is compared with the float64 reference that rasters WORLD coordinates — no oracle, no restatement.

The tools compute their matrices in their own precision: submapwin::relativePose evaluates R_i^T R_j and R_i^T (t_j - t_i) in
double from the float32 rows and rounds to float (R_i^T where the reference inverts the rounded matrix: 1e-7 of the
coordinates), and batch_posed_bev_gen builds its matrix with sinf / cosf of the float yaw.  Both stay below 1e-5 m on this
world; MARGIN = 1e-3 m, by which the filter keeps every point away from a bin, layer or height edge, covers that.  The
filter covers every key frame compared: key frames 2, 3 and 4 at half window 2 are the maps A, K and B, and frame 3 under the
two pose rows are the grids ("cli", k).

batch_posed_bev_gen reads poses as tx ty tz yaw_deg only, so its rows are general in those four numbers; matrices with roll
and pitch reach bev_posed_bev_batch in test_raster_world_gpu.py."""
import os
import subprocess

import numpy as np
import pytest

import bev_amd
import pcd_util
import raster_world_cases as rw

pytestmark = pytest.mark.gpu
HOST = bev_amd.PKG_DIR / "host"
SENSOR = "HDL_64E"            # the tools raster at interval 1.0: this sensor's configuration
KEYS = {2: "A", 3: "K", 4: "B"}


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    c = rw.case(SENSOR)
    assert c.interval == 1.0
    root = tmp_path_factory.mktemp("kf_raster_world")
    (root / "non_ground_point_cloud").mkdir()
    for i, f in enumerate(c.frames):
        pcd_util.write_pcd_binary(root / "non_ground_point_cloud" / f"{i:06d}.pcd", f)
    rows = []
    for i, P in enumerate(c.P):
        assert np.array_equal(P, P.astype(np.float32).astype(np.float64))
        rows.append(",".join([str(i)] + [repr(float(v)) for v in P[:3, 3]] + ["0", "0", "0"] + [repr(float(v)) for v in P[:3, :3].reshape(9)]))
    (root / "keyframe_pose.csv").write_text("\n".join(rows) + "\n")
    return c, root


def _run(tool, args, root):
    env = dict(os.environ, BEV_MAX_POINTS="4096", BEV_BATCH="3")
    r = subprocess.run([str(HOST / tool), str(root), *args], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("Done."), r.stdout


def _csv_u8(path):
    return np.array([[int(v) for v in l.split(",")] for l in path.read_text().splitlines()], np.uint8)


def test_batch_submap_bev_gen_writes_the_float64_worlds_images(tree):
    c, root = tree
    _run("batch_submap_bev_gen", [SENSOR, "2"], root)
    for key, name in KEYS.items():
        multi, single = c.reference(name)
        got = np.frombuffer((root / "output_submap_bev" / "binary" / f"{key:06d}.bin").read_bytes(), np.uint8)
        rw.compare_bytes(got.reshape(multi.shape), multi, f"key frame {key}, .bin")
        rw.compare_bytes(_csv_u8(root / "output_submap_bev" / "csv" / f"{key:06d}.csv"), single, f"key frame {key}, .csv")
        assert multi.any() and single.any()


def test_batch_submap_cloud_manip_writes_the_float64_worlds_grids(tree):
    c, root = tree
    _run("batch_submap_cloud_manip", [SENSOR, "2"], root)
    tol = c.tol()
    assert tol <= rw.CAP
    for key, name in KEYS.items():
        want = c.reference_float(name, True)
        got = np.array([[float(v) for v in l.split(",")] for l in (root / "output_submap_bvm" / f"{key:06d}.csv").read_text().splitlines()])
        assert got.shape == want.shape and np.array_equal(got > 0, want > 0), key
        # '%.4g': half a unit of the fourth significant digit of the value printed (of the larger of the two at a power of ten)
        digit = np.where(want > 0, 0.5 * 10.0 ** (np.floor(np.log10(np.maximum(np.maximum(want, got), 1e-30))) - 3), 0.0)
        off = np.abs(got - want)
        print(f"key frame {key}: {int((want > 0).sum())} cells, at most {off.max():.2e} from the float64 world (tol {tol:.2e} + print precision)")
        assert (off <= tol + digit * (1 + 1e-9)).all(), (key, float((off - digit).max()))


def test_batch_posed_bev_gen_writes_the_float64_worlds_images(tree):
    c, root = tree
    poses = root / "poses.txt"
    poses.write_text("# tx ty tz yaw_deg\n" + "".join(" ".join(repr(float(v)) for v in row) + "\n" for row in rw.CLI_POSES))
    _run("batch_posed_bev_gen", [SENSOR, str(poses)], root)
    for k in range(len(rw.CLI_POSES)):
        multi, single = c.reference(("cli", k))
        got = np.frombuffer((root / "output_posed_bev" / "binary" / f"000003_{k:02d}.bin").read_bytes(), np.uint8)
        rw.compare_bytes(got.reshape(multi.shape), multi, f"frame 3, pose {k}, .bin")
        rw.compare_bytes(_csv_u8(root / "output_posed_bev" / "csv" / f"000003_{k:02d}.csv"), single, f"frame 3, pose {k}, .csv")
        assert multi.any() and single.any()
