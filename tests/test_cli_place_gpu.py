"""GPU: batch_place_retrieval (host C++ over bev_place_retrieval_batch) end to end, on the clouds of
ground_truth_cases.py (§6o) written as PCD files with a pose file: its match list parses with the project's reader and equals
the Python binding's hits at half windows 0 and 2, top_k 3 gives three lines per query in rank order, and a missing directory
exits non-zero."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import bev_amd
import ground_truth_cases as gt
import pcd_util

pytestmark = pytest.mark.gpu
CLI = Path(bev_amd.PKG_DIR) / "host" / "batch_place_retrieval"
EXCLUDE = 2


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    S = gt.setup(round_poses=True)
    root = tmp_path_factory.mktemp("kf_place")
    (root / "non_ground_point_cloud").mkdir()
    for i, c in enumerate(S["clouds"]):
        pcd_util.write_pcd_binary(root / "non_ground_point_cloud" / f"{i:06d}.pcd", c)
    rows = [",".join([str(i)] + [repr(float(v)) for v in P[:3, 3]] + ["0", "0", "0"] + [repr(float(v)) for v in P[:3, :3].reshape(9)])
            for i, P in enumerate(S["poses"])]
    (root / "keyframe_pose.csv").write_text("\n".join(rows) + "\n")
    return dict(S=S, root=root)


@pytest.fixture(scope="module")
def reader(tmp_path_factory):
    """loadMatchResults (host/MatchResults.cpp, what every registration tool reads its matches with) behind a small driver"""
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the build toolchain"
    d = tmp_path_factory.mktemp("reader")
    (d / "drv.cpp").write_text('#include "Registration.h"\n#include <cstdio>\nint main(int, char **argv) {\n'
                               '  try { for (const auto &m : loadMatchResults(argv[1])) std::printf("%d %d %.9g\\n", m.query_idx,'
                               ' m.match_idx, (double)m.angle_guess); } catch (const std::exception &e) { std::printf("ERR %s\\n",'
                               ' e.what()); return 3; }\n  return 0;\n}\n')
    host = Path(bev_amd.PKG_DIR) / "host"
    subprocess.run([gxx, "-std=c++17", "-O1", "-I", str(host), str(d / "drv.cpp"), str(host / "MatchResults.cpp"), "-o", str(d / "drv")],
                   check=True)

    def read(path):
        out = subprocess.run([str(d / "drv"), str(path)], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout
        return [(int(a), int(b), np.float32(c)) for a, b, c in (l.split() for l in out.stdout.splitlines())]
    return read


def _relative12(Pi, Pj):
    """submapwin::relativePose: R_i^T R_j and R_i^T (t_j - t_i) in double from the float rows, rounded to float"""
    m = np.zeros((3, 4))
    m[:, :3] = Pi[:3, :3].T @ Pj[:3, :3]
    m[:, 3] = Pi[:3, :3].T @ (Pj[:3, 3] - Pi[:3, 3])
    return m.astype(np.float32).reshape(12)


def _binding_hits(S, half, top_k):
    n = len(S["clouds"])
    offs, ef, ep = [0], [], []
    for i in range(n):
        for j in range(max(0, i - half), min(n - 1, i + half) + 1):
            ef.append(j)
            ep.append(np.eye(3, 4, dtype=np.float32).reshape(12) if j == i else _relative12(S["poses"][i], S["poses"][j]))
        offs.append(len(ef))
    limit = np.maximum(0, np.arange(n) - EXCLUDE + 1).astype(np.int32)
    ctx = bev_amd.BevContext(bev_amd.params_for_sensor("HDL_64E"), device=0, max_batch=4)
    try:
        return ctx.place_retrieval_batch(S["clouds"], top_k, limit, None, np.array(offs, np.uint64), np.array(ef, np.int32),
                                         np.array(ep, np.float32))
    finally:
        ctx.close()


def _run(root, *args):
    return subprocess.run([str(CLI), str(root), "HDL_64E", *args], capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("half,top_k", [(0, 1), (2, 1), (2, 3)])
def test_match_list_equals_the_binding(tree, reader, half, top_k):
    assert CLI.exists(), "host CLI not built"
    S, root = tree["S"], tree["root"]
    (root / "place_retrieval").mkdir(exist_ok=True)
    (root / "place_retrieval" / "stale.txt").write_text("must be removed")
    r = _run(root, str(half), str(EXCLUDE), *([str(top_k)] if top_k != 1 else []))
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(f.name for f in (root / "place_retrieval").iterdir()) == ["match_detail.csv", "match_result.txt"]
    hits = _binding_hits(S, half, top_k).reshape(-1)
    kept = hits[hits["match_idx"] >= 0]
    n = len(S["clouds"])
    assert len(kept) == sum(min(top_k, max(0, q - EXCLUDE + 1)) for q in range(n)) and len(kept) > 0
    assert reader(root / "place_retrieval" / "match_result.txt") == [(int(h["query_idx"]), int(h["match_idx"]), h["angle_guess"]) for h in kept]
    detail = (root / "place_retrieval" / "match_detail.csv").read_text().splitlines()
    assert detail[0] == "query_idx,match_idx,shift,angle_guess,distance" and len(detail) == len(kept) + 1
    for line, h in zip(detail[1:], kept):
        q, m, shift, ang, dist = line.split(",")
        assert (int(q), int(m), int(shift), np.float32(ang), float(dist)) == (h["query_idx"], h["match_idx"], h["shift"], h["angle_guess"], h["distance"])
    if top_k == 3:  # rank order within a query: the distances do not decrease
        for q in range(n):
            d = kept["distance"][kept["query_idx"] == q]
            assert len(d) == min(3, max(0, q - EXCLUDE + 1)) and (np.diff(d) >= 0).all()
    if half == 2:   # a map holds more than its key frame: the hits differ from those of the frames alone
        assert hits.tobytes() != _binding_hits(S, 0, top_k).reshape(-1).tobytes()


def test_max_distance_and_refusals(tree, tmp_path):
    root = tree["root"]
    r = _run(root, "0", str(EXCLUDE), "1", "-1")
    assert r.returncode == 0 and (root / "place_retrieval" / "match_result.txt").read_text() == ""
    assert _run(tmp_path / "missing", "0").returncode != 0
    assert _run(root, "x").returncode != 0 and _run(root, "0", "-1").returncode != 0 and _run(root, "0", "2", "65").returncode != 0
    assert subprocess.run([str(CLI)], capture_output=True, text=True, timeout=60).returncode != 0
