"""GPU: BEV_PAIR_SEARCH_GRID of batch_top_part_registration and batch_whole_registration end to end, on a small
seeded directory: four clouds (wall segments over a lattice of 17 000 points, one point per voxel at leaf 0.2, so that every fine
target has more than 16 384 points, above the fixed grid's 128 x 128 cells) a few centimetres apart.  Unset, 0, 256 and 256,128
write identical files and, the times apart, identical lines: the search does not depend on its grid."""
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
TOOLS = {"batch_top_part_registration": "icp_precision_report.txt", "batch_whole_registration": "icp_precision_report_3d_icp_directly.txt"}
N = 4


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("pairs")
    pcd = root / "pcd"
    pcd.mkdir()
    world_walls = tc.wall_cloud(1500, 9970)
    for i in range(N):
        floor = vc.lattice(17000, 9980 + i)
        floor["z"] -= np.float32(3.0)
        walls = world_walls.copy()
        walls["x"] -= np.float32(0.03125 * i)                     # the same walls seen from a place a little further on
        walls["y"] -= np.float32(0.0625 * i)
        pcd_util.write_pcd_binary(pcd / f"{i:06d}.pcd", np.concatenate([walls, floor]))
    (root / "matches.txt").write_text("0 2 0.0\n3 3 1.0\n1 0 -1.0\n3 2 0.5\n1 2 0.0\n")
    return root


def _run(tool, root, cwd, grid):
    env = {k: v for k, v in os.environ.items() if k != "BEV_PAIR_SEARCH_GRID"}
    if grid is not None:
        env["BEV_PAIR_SEARCH_GRID"] = grid
    r = subprocess.run([str(HOST / tool), str(root / "matches.txt"), str(root / "pcd")], cwd=cwd, capture_output=True, text=True,
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
    print(tool, outs["unset"][0], outs["unset"][1][TOOLS[tool]].decode())
    assert re.search(r"count_success: [1-9]", outs["unset"][0])      # matches that succeed: the targets are really searched
    assert TOOLS[tool] in outs["unset"][1]
    for name in ("zero", "wide", "two"):
        assert outs[name] == outs["unset"], name
