"""GPU: batch_aligned_registration (the whole tool's chain against windows with the translation guess ahead of every chunk's fine
stage) end to end on test_cli_submap_registration_gpu.py's tree of PCD files: alignment_detail.csv and the report
equal what the binding's chain gives for the same matches, at half windows 0 and 2 and at two chunk sizes; BEV_ALIGN is parsed
and refused; batch_submap_registration on the same inputs writes what it wrote."""
import os
import subprocess

import numpy as np
import pytest

import bev_amd
import fineicp_lib as fl
import reg_cases as rc
import submap_reg_cases as sc
import test_cli_submap_registration_gpu as base
from bev_amd import ALIGN_DETAIL_DTYPE, ICP_RESULT_DTYPE, align_params
from test_cli_submap_registration_gpu import tree  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
HEADER = "query,match,flip,chosen,dx,dy,k,score,eq,ec,off_x,off_y,fitness,tx,ty\n"
ENV = "64,1.0,8,1,2.0"


def _binding(tree, rows, half, prm):
    """(fine, table (n, 2), best, detail (n, 2)) of the rows through the device-resident calls, nothing between them"""
    import torch

    clouds = tree["clouds"]
    maps = sc.Maps()
    for q, t, a in rows:
        maps.add([(j, sc.IDENTITY if j == t else base._relative(t, j)) for j in range(max(0, t - half), min(base.N - 1, t + half) + 1)])
    m = sc.matches([(q, k, a) for k, (q, t, a) in enumerate(rows)])
    n = len(m)
    ctx = bev_amd.BevContext(bev_amd.params_for_sensor("HDL_64E"), device=0, max_batch=2, max_points=4096)
    try:
        offs = np.r_[0, np.cumsum([len(c) for c in clouds])].astype(np.uint64)
        dev = torch.device("cuda:0")
        z = lambda b: torch.zeros(max(b, 1), dtype=torch.uint8, device=dev)
        d_clouds = torch.from_numpy(rc.packed(clouds).view(np.uint8).reshape(-1).copy()).to(dev)
        d_grids, d_energy = z(n * prm.grid * prm.grid), z(4 * n)
        d_tab, d_best, d_det = z(2 * n * ICP_RESULT_DTYPE.itemsize), z(4 * n), z(2 * n * ALIGN_DETAIL_DTYPE.itemsize)
        d_res = z(n * ICP_RESULT_DTYPE.itemsize)
        torch.cuda.synchronize()
        ctx.align_grid_device(len(clouds), d_clouds.data_ptr(), offs, d_grids.data_ptr(), d_energy.data_ptr(), prm, *maps.arrays())
        ctx.align_hits_device(len(clouds), d_clouds.data_ptr(), offs, n, d_grids.data_ptr(), d_energy.data_ptr(), m,
                              d_tab.data_ptr(), d_best.data_ptr(), d_det.data_ptr(), prm)
        ctx.submap_voxel_registration_device(len(clouds), d_clouds.data_ptr(), offs, *maps.arrays(), m, d_res.data_ptr(), 0.0,
                                             d_tab.data_ptr(), d_best.data_ptr(), params=fl.params(**fl.WHOLE))
        ctx.synchronize()
        return (d_res.cpu().numpy().view(ICP_RESULT_DTYPE)[:n].copy(), d_tab.cpu().numpy().view(ICP_RESULT_DTYPE)[: 2 * n].reshape(n, 2).copy(),
                d_best.cpu().numpy().view(np.int32)[:n].copy(), d_det.cpu().numpy().view(ALIGN_DETAIL_DTYPE)[: 2 * n].reshape(n, 2).copy())
    finally:
        ctx.close()


def _csv(rows, table, best, det):
    out = HEADER
    for k, (q, t, _) in enumerate(rows):
        for flip in (0, 1):
            d, r = det[k, flip], table[k, flip]
            out += "%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%.9g,%.9g,%.17g,%.9g,%.9g\n" % (
                q, t, flip, int(best[k] == flip), d["dx"], d["dy"], d["k"], d["score"], d["eq"], d["ec"], float(d["off_x"]),
                float(d["off_y"]), float(r["fitness"]), float(r["T"][3]), float(r["T"][7]))
    return out


def _run(tool, args, cwd, env=None, ok=True):
    e = dict(os.environ)
    e.pop("BEV_ALIGN", None)
    e.update(env or {})
    r = subprocess.run([str(base.HOST / tool), *[str(a) for a in args]], cwd=cwd, capture_output=True, text=True, timeout=600, env=e)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r


@pytest.mark.parametrize("half", [0, 2])
def test_tool_writes_what_the_binding_gives(tree, tmp_path, half):
    root, rows = tree["root"], tree["rows"]
    prm = align_params(64, 1.0, 8, 1, 2.0)
    fine, table, best, det = _binding(tree, rows, half, prm)
    csv = _csv(rows, table, best, det)
    for k in range(len(rows)):
        print(rows[k], int(best[k]), det[k, best[k]], float(fine[k]["fitness"]))
    m = sc.matches(rows)
    report = "".join(fl.report_line(fine[k]["T"], fl.tool_guess(float(m["angle_guess"][k]))) for k in range(len(m))
                     if not fine[k]["fitness"] > 1.5)
    for chunk in ("6", None):
        d = tmp_path / f"chunk{chunk}"
        d.mkdir()
        r = _run("batch_aligned_registration", [root / "matches.txt", root, half] + ([chunk] if chunk else []), d, {"BEV_ALIGN": ENV})
        assert (d / "alignment_detail.csv").read_text() == csv, chunk
        assert (d / "icp_precision_report_submap.txt").read_text() == report, chunk
        assert (d / "icp_precision_report_3d_icp_directly.txt").read_bytes() == b""
        assert base._summary(fine["fitness"]) in r.stdout
    assert csv.count("\n") == 2 * len(rows) + 1 and (det["score"] > 0).any()
    assert report.count("\n") >= 5  # (as many successes as the tool without the step is asked for on this tree)
    # the defaults are what an unset or empty BEV_ALIGN gives
    dflt = _csv(rows, *_binding(tree, rows, half, align_params())[1:])
    for env in ({}, {"BEV_ALIGN": ""}):
        d = tmp_path / f"default{len(env)}"
        d.mkdir()
        _run("batch_aligned_registration", [root / "matches.txt", root, half], d, env)
        assert (d / "alignment_detail.csv").read_text() == dflt


def test_the_tool_without_the_step_writes_what_it_wrote(tree, tmp_path):
    """batch_submap_registration passes no alignment parameters: the whole tool's bytes at half window 0, with or without
    BEV_ALIGN in its environment, and no detail file"""
    root = tree["root"]
    outs = []
    for name, env in (("plain", {}), ("env", {"BEV_ALIGN": ENV}), ("bad", {"BEV_ALIGN": "x"})):
        d = tmp_path / name
        d.mkdir()
        outs.append((d, _run("batch_submap_registration", [root / "matches.txt", root, 0], d, env)))
        assert not (d / "alignment_detail.csv").exists()
    (tmp_path / "whole").mkdir()
    whole = _run("batch_whole_registration", [root / "matches.txt", root / "non_ground_point_cloud"], tmp_path / "whole")
    for d, r in outs:
        assert base._stdout_without_times(r) == base._stdout_without_times(whole)
        assert (d / "icp_precision_report_submap.txt").read_bytes() == (outs[0][0] / "icp_precision_report_submap.txt").read_bytes()


@pytest.mark.parametrize("text", ["x", "64", "64,1.0,8,1", "64,1.0,8,1,2.0,1", "64,1.0,8,1,2.0 ", " 64,1.0,8,1,2.0", "63,1.0,8,1,2.0",
                                  "14,1.0,2,1,2.0", "130,1.0,8,1,2.0", "64,0,8,1,2.0", "64,-1,8,1,2.0", "64,nan,8,1,2.0", "64,inf,8,1,2.0",
                                  "64,1.0,0,1,2.0", "64,1.0,17,1,2.0", "32,1.0,9,1,2.0", "64,1.0,8,-1,2.0", "64,1.0,8,4,2.0",
                                  "64,1.0,8,1,-2.0", "64,1.0,8,1,nan", "64,1.0,8.5,1,2.0", "64;1.0;8;1;2.0"])
def test_bev_align_refused_before_any_work(tree, tmp_path, text):
    r = _run("batch_aligned_registration", [tree["root"] / "matches.txt", tree["root"], 0], tmp_path, {"BEV_ALIGN": text}, ok=False)
    assert r.returncode == 1 and f"BEV_ALIGN '{text}'" in r.stderr and "Usage: batch_aligned_registration" in r.stderr
    assert not (tmp_path / "alignment_detail.csv").exists()


def test_too_few_arguments(tmp_path):
    r = subprocess.run([str(base.HOST / "batch_aligned_registration"), "a", "b"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Usage: batch_aligned_registration" in r.stderr
