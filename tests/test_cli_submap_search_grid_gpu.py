"""GPU: BEV_SUBMAP_SEARCH_GRID of batch_submap_registration and batch_submap_top_part_registration end to end,
on a small seeded directory: seven clouds (wall segments over a lattice of 3600 points, one point per voxel at leaf 0.2) under
poses a few centimetres apart, so that every window of half width 2 is a fine map of more than 16 384 points, above the fixed
grid's 128 x 128 cells.  Unset, 0, 256 and 256,128 write identical files and, the times apart, identical lines: the search does
not depend on its grid."""
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import bev_amd
import pcd_util
import submap_top_cases as tc
import submap_vox_cases as vc

pytestmark = pytest.mark.gpu
HOST = Path(bev_amd.PKG_DIR) / "host"
TOOLS = {"batch_submap_registration": "icp_precision_report_submap.txt", "batch_submap_top_part_registration": "icp_precision_report.txt"}
N = 7
VARS = ("BEV_SUBMAP_SEARCH_GRID", "BEV_SUBMAP_PN_LEAF", "BEV_SUBMAP_TOP_UNION", "BEV_SUBMAP_REG_GROUP")


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("kf")
    pcd = root / "non_ground_point_cloud"
    pcd.mkdir()
    world_walls = tc.wall_cloud(1500, 9950)
    for i in range(N):
        floor = vc.lattice(3600, 9960 + i)
        floor["z"] -= np.float32(3.0)
        walls = world_walls.copy()
        walls["x"] -= np.float32(0.03125 * i)                     # the same walls seen from pose i
        walls["y"] -= np.float32(0.0625 * i)
        pcd_util.write_pcd_binary(pcd / f"{i:06d}.pcd", np.concatenate([walls, floor]))
    pose = lambda i: ",".join([str(i), repr(0.03125 * i), repr(0.0625 * i), "0.0", "0", "0", "0", "1.0", "0.0", "0.0", "0.0", "1.0", "0.0",
                               "0.0", "0.0", "1.0"])
    (root / "keyframe_pose.csv").write_text("\n".join(pose(i) for i in range(N)) + "\n")
    (root / "matches.txt").write_text("0 2 0.0\n3 3 1.0\n5 4 -1.0\n6 2 0.5\n1 5 0.0\n")
    return root


def _run(tool, root, cwd, grid):
    env = {k: v for k, v in os.environ.items() if k not in VARS}
    if grid is not None:
        env["BEV_SUBMAP_SEARCH_GRID"] = grid
    r = subprocess.run([str(HOST / tool), str(root / "matches.txt"), str(root), "2"], cwd=cwd, capture_output=True, text=True,
                       timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = re.sub(r"(\[TIME\] Avg Tiempo for \S+ Stage \(\w+\): )\S+", r"\1T", r.stdout)
    return lines, {p.name: p.read_bytes() for p in sorted(Path(cwd).iterdir()) if p.is_file()}


@pytest.mark.parametrize("tool", sorted(TOOLS))
def test_the_output_does_not_depend_on_the_search_grid(tool, tree, tmp_path):
    outs = {}
    for name, grid in (("unset", None), ("zero", "0"), ("wide", "256"), ("two", "256,128")):
        d = tmp_path / name
        d.mkdir()
        outs[name] = _run(tool, tree, d, grid)
    report = outs["unset"][1][TOOLS[tool]]
    print(tool, outs["unset"][0], report.decode())
    assert report.count(b"\n") >= 3                                 # matches that succeed: the maps are really searched
    for name in ("zero", "wide", "two"):
        assert outs[name] == outs["unset"], name
