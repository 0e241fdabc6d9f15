"""GPU: the batch registration CLIs (host/batch_top_part_registration, host/batch_whole_registration) on PCD files of
the BEV path's ordered clouds: their report files and summary counts equal the checker chain's (front end, coarse ICP,
fine ICP, report maths: tests/regfront, tests/icp, tests/fineicp), at two chunk sizes."""
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import bev_amd
import fineicp_lib as fl
import icp_lib as il
import pcd_util
import regfront_lib as rl
from bev_amd import synth

pytestmark = pytest.mark.gpu
HOST = Path(bev_amd.PKG_DIR) / "host"
THREADS = min(16, os.cpu_count() or 4)
F32 = np.float32


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    fl.build()
    il.build()
    rl.build()
    p = bev_amd.params_for_sensor("HDL_64E")
    rng = np.random.default_rng(31)
    F0 = 8
    base = [synth.sweep(p, 700 + i, keep=0.98, n_dup=2000) for i in range(F0)]
    ctx = bev_amd.BevContext(p, device=0, max_batch=4, max_points=max(len(f) for f in base))
    try:
        yaw = rng.uniform(-15, 15, F0).astype(F32)
        tr = rng.uniform(-1, 1, (F0, 2)).astype(F32)
        moved = [ctx.transform_cloud(base[i], bev_amd.yaw_translate_matrix(float(tr[i, 0]), float(tr[i, 1]), 0.0,
                                                                           float(yaw[i]))) for i in range(F0)]
        ordered = [ctx.process_batch([f], want_multi=False, want_single=False)[0][0] for f in base + moved]
    finally:
        ctx.close()
    d = tmp_path_factory.mktemp("reg")
    pcd = d / "pcd"
    pcd.mkdir()
    ids = [3 + 2 * k for k in range(len(ordered))]  # file names are not frame positions
    for k, o in enumerate(ordered):
        pcd_util.write_pcd_binary(pcd / f"{ids[k]:06d}.pcd", o)
    m = [(ids[i], ids[F0 + i], float(F32(yaw[i] + rng.uniform(-2, 2)))) for i in range(F0)]  # float32 values: exact in text
    m += [(ids[i], ids[(i + 1) % F0], float(F32(rng.uniform(-3, 3)))) for i in range(F0)]
    (d / "matches.txt").write_text("".join(f"{q} {t} {a!r}\n" for q, t, a in m))
    # the checker chain on the same clouds
    pos = {f: k for k, f in enumerate(ids)}
    mk = [(pos[q], pos[t], np.float32(a)) for q, t, a in m]
    pn = [rl.chain(o) for o in ordered]
    coarse, best = il.coarse(pn, mk, threads=THREADS)
    guesses = [coarse[k, best[k]]["T"].reshape(4, 4) for k in range(len(mk))]
    top = fl.fine(ordered, mk, guesses, fl.params(**fl.FINE), threads=THREADS)
    whole = fl.fine(ordered, mk, None, fl.params(**fl.WHOLE), threads=THREADS)
    lines = "".join(fl.report_line(top[k]["T"], guesses[k]) for k in range(len(mk)) if not top[k]["fitness"] > 1.5)
    return dict(dir=d, top=top, whole=whole, lines=lines)


def _summary(fit):
    ok = int((~(fit > 1.5)).sum())
    bad = len(fit) - ok
    return f"count_success: {ok}, count_failure: {bad}, SR: {'%g' % float(F32(ok) / F32(ok + bad))}. "


@pytest.mark.parametrize("max_frames", ["256", "3"])
def test_top_part_cli_equals_the_checker_chain(scene, max_frames, tmp_path):
    d = scene["dir"]
    r = subprocess.run([str(HOST / "batch_top_part_registration"), str(d / "matches.txt"), str(d / "pcd"), max_frames],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "icp_precision_report.txt").read_text() == scene["lines"]
    assert _summary(scene["top"]["fitness"]) in r.stdout
    assert re.search(r"\[TIME\] Avg Tiempo for 1st Stage \(coarse\): ", r.stdout)
    assert re.search(r"\[TIME\] Avg Tiempo for 2nd Stage \(fine\): ", r.stdout)
    assert scene["lines"].count("\n") > 0


@pytest.mark.parametrize("max_frames", ["256", "2"])
def test_whole_cli_equals_the_checker_chain(scene, max_frames, tmp_path):
    d = scene["dir"]
    r = subprocess.run([str(HOST / "batch_whole_registration"), str(d / "matches.txt"), str(d / "pcd"), max_frames],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "icp_precision_report_3d_icp_directly.txt").read_text() == ""  # created, never written
    assert _summary(scene["whole"]["fitness"]) in r.stdout
    assert (~(scene["whole"]["fitness"][:8] > 1.5)).all()  # the moved copies register


def test_unreadable_file_exits_1(scene, tmp_path):
    (tmp_path / "m.txt").write_text("1 999999 0.0\n")
    for tool in ("batch_top_part_registration", "batch_whole_registration"):
        r = subprocess.run([str(HOST / tool), str(tmp_path / "m.txt"), str(scene["dir"] / "pcd")], cwd=tmp_path,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "Cloud NOT load file" in r.stderr
