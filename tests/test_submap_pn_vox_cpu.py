"""CPU: scan-to-map coarse ICP against maps thinned over their union without a GPU — the two entry points in the
library and the bindings; the tool's BEV_SUBMAP_PN_LEAF; the host plan with its byte model, by the stand-alone
tests/submappncheck, plain and as a second program under the address and undefined-behaviour sanitizers; the condition the
seeded list puts on its inputs, on the checker's results alone; and the entry-order pair: two orders of a map's entries whose
union is the same but whose centroids differ, because a float32 sum depends on its order."""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import bev_amd
import icp_lib
import regfront_lib as rf
import submap_coarse_cases as cc
import submap_pn_vox_cases as pv
import submap_reg_cases as sc

DIR = Path(__file__).resolve().parent / "submappncheck"
TOP = bev_amd.PKG_DIR / "host" / "batch_submap_top_part_registration"
WHOLE = bev_amd.PKG_DIR / "host" / "batch_submap_registration"
INVALID = -1
F32 = np.float32
SANITIZE = "-fsanitize=address,undefined -fno-omit-frame-pointer"
NEW = ("bev_submap_coarse_voxel_registration_device_resident", "bev_submap_pn_cloud_device_resident")


@pytest.fixture(scope="module", autouse=True)
def _checkers():
    icp_lib.build()
    rf.build()


# ---- exports, bindings ------------------------------------------------------------------------------------------------------------
def test_the_two_entry_points_are_exported_and_bound_and_refuse_a_null_context():
    lib = bev_amd.load_lib()
    assert set(NEW) <= set(bev_amd.ABI_SYMBOLS) and all(hasattr(lib, n) for n in NEW)
    for name in ("submap_coarse_voxel_registration_device", "submap_pn_cloud_device"):
        assert hasattr(bev_amd.BevContext, name), name
    assert lib.bev_abi_version() == 1                      # the change only adds
    header = (bev_amd.REPO_DIR / "include" / "bev_mi355x.h").read_text()
    assert all(f"int {n}(" in header for n in NEW)
    moffs = np.array([0, 1], dtype=np.uint64)
    eframe = np.zeros(1, dtype=np.int32)
    epose = sc.IDENTITY.reshape(1, 12).copy()
    pn = np.zeros((4, 12), F32)
    counts = np.array([4], np.uint32)
    m = sc.matches([(0, 0, 0.0)])
    out = np.full(2 * bev_amd.ICP_RESULT_DTYPE.itemsize, 0xA5, dtype=np.uint8)
    best = np.full(1, 0x5A5A5A5A, dtype=np.int32)
    rows, n_rows = np.full(4 * 48, 0xA5, dtype=np.uint8), np.full(4, 0xA5, dtype=np.uint8)
    u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    assert lib.bev_submap_coarse_voxel_registration_device_resident(
        None, 1, pn.ctypes.data, 4, counts.ctypes.data, 0.2, 2.0, None, 1, u64(moffs), eframe.ctypes.data, epose.ctypes.data, 1,
        m.ctypes.data, None, out.ctypes.data, best.ctypes.data) == INVALID
    assert lib.bev_submap_pn_cloud_device_resident(
        None, 1, pn.ctypes.data, 4, counts.ctypes.data, 0.2, 2.0, None, 1, u64(moffs), eframe.ctypes.data, epose.ctypes.data, 4,
        rows.ctypes.data, n_rows.ctypes.data) == INVALID
    assert (out == 0xA5).all() and best[0] == 0x5A5A5A5A and (rows == 0xA5).all() and (n_rows == 0xA5).all()


# ---- the tool's variable ------------------------------------------------------------------------------------------------------------
def _run(tool, *args, cwd=None, pn_leaf=None):
    env = {k: v for k, v in os.environ.items() if k != "BEV_SUBMAP_PN_LEAF"}
    if pn_leaf is not None:
        env["BEV_SUBMAP_PN_LEAF"] = pn_leaf
    return subprocess.run([str(tool), *[str(a) for a in args]], capture_output=True, text=True, timeout=60, cwd=cwd, env=env)


def test_the_tool_reads_its_variable_and_refuses_what_is_no_finite_number_before_any_gpu_work(tmp_path):
    assert TOP.exists() and WHOLE.exists(), "host CLI not built"
    (tmp_path / "non_ground_point_cloud").mkdir()
    (tmp_path / "m.txt").write_text("0 0 0.0\n")
    for text in ("-1", "nan", "0.2x", "-0.5", "inf", "leaf", "1e99", " "):
        r = _run(TOP, tmp_path / "m.txt", tmp_path, 1, cwd=tmp_path, pn_leaf=text)
        assert r.returncode == 1 and r.stdout == "", (text, r.stdout)
        assert f"BEV_SUBMAP_PN_LEAF '{text}': expected a finite number >= 0" in r.stderr, (text, r.stderr)
        assert "bev_create" not in r.stderr and "HIP" not in r.stderr and "keyframe_pose.csv" not in r.stderr
        assert not (tmp_path / "icp_precision_report.txt").exists()                 # refused before anything is created
    for text in (None, "", "0", "0.0", "0.5", "1e-3"):                              # accepted: the next complaint is the pose file's
        r = _run(TOP, tmp_path / "m.txt", tmp_path, 1, cwd=tmp_path, pn_leaf=text)
        assert r.returncode == 1 and "BEV_SUBMAP_PN_LEAF" not in r.stderr and "keyframe_pose.csv" in r.stderr, (text, r.stderr)
    r = _run(TOP, cwd=tmp_path, pn_leaf="0.5")                                      # the usage line stays what it is
    assert r.returncode == 1 and r.stderr.startswith(
        "Usage: batch_submap_top_part_registration <match_result_text_file> <keyframes_root_dir> <half_window> [<chunk> [<map_leaf>]]")
    r = _run(WHOLE, tmp_path / "m.txt", tmp_path, 1, cwd=tmp_path, pn_leaf="nan")   # no coarse stage: the variable is not read
    assert r.returncode == 1 and "BEV_SUBMAP_PN_LEAF" not in r.stderr and "keyframe_pose.csv" in r.stderr


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------
def _build_and_run(program):
    """a fresh build of one of the two programs, its run, and a clean tree"""
    try:
        subprocess.run(["make", "-C", str(DIR), "clean"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        r = subprocess.run(["make", "-C", str(DIR), program], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            return r, None
        return r, subprocess.run([str(DIR / program)], capture_output=True, text=True, timeout=300)
    finally:
        subprocess.run(["make", "-C", str(DIR), "clean"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _assert_ok(run):
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().splitlines()
    assert [l for l in lines if l.startswith("ok:")] == lines[-1:] and "PLAN" not in run.stdout, run.stdout
    words = lines[-1].replace(",", "").split()   # ok: submappncheck: P plans, T of them thinned PointNormal plans, G launch groups, K of ...
    plans, thinned, groups, oversize = int(words[2]), int(words[4]), int(words[10]), int(words[13])
    assert plans == 2000 and thinned == 250 * 2 and groups > plans and 0 < oversize < groups


def test_the_plan_keeps_its_byte_models_and_existing_calls_plan_as_before():
    built, run = _build_and_run("submappncheck")
    assert built.returncode == 0, built.stdout
    _assert_ok(run)


def test_the_same_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    r = subprocess.run(["gcc", *SANITIZE.split(), "-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("the sanitizer runtime is not installed: " + (r.stderr.strip().splitlines() or ["gcc failed"])[-1])
    built, run = _build_and_run("submappncheck_san")       # a stand-alone host program, run directly
    assert built.returncode == 0, built.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr
    _assert_ok(run)


def test_the_checkers_group_count_restates_the_plans_byte_model():
    S = pv.seeded_list()
    n_groups, alone = pv.group_count(S["maps"], S["m"], S["stride"], 150000)
    assert n_groups >= 10 and 1 <= alone < len(S["maps"])
    assert pv.group_count(S["maps"], S["m"], S["stride"], 1 << 40) == (1, 0)


# ---- the seeded list --------------------------------------------------------------------------------------------------------------------
def test_the_seeded_list_meets_its_condition_on_the_checker():
    S = pv.seeded_list()
    frames, maps, m, H = S["frames"], S["maps"], S["m"], S["H"]
    sizes = [len(f) for f in frames[:H]]
    assert set(pv.LIST_SIZES) <= set(sizes) and len(sizes) == 20 and min(sizes) >= 63 and max(sizes) == 512 > S["stride"]
    flat = lambda t: ((t[:, 6] == 0) | np.isnan(t[:, 4])).all()                        # nz = 0 exactly, but for a lone point's NaNs
    assert all((f[:, 2] == 0).all() and flat(f) for f in frames)                    # what the front end emits
    assert sorted({len(maps.entries(g)) for g in range(len(maps))}) == [1, 2, 3, 4, 5, 6]
    assert len(m) == 2 * H                                                          # two guesses each: 80 problems
    concat = sum(len(cc.target(frames, maps.entries(g), S["stride"])) for g in range(len(maps)))
    for leaf in pv.LEAVES:
        res, best = pv.seeded_expected(leaf)
        tgt = pv.seeded_targets(leaf)
        share = pv.condition_share(res)
        nans = sum(int(np.isnan(t[:, 4]).sum()) for t in tgt)
        print(f"leaf {leaf}: {share:.3f} of {res.size} problems keep correspondences for two iterations or more; {concat} rows "
              f"thinned to {sum(len(t) for t in tgt)}, {nans} NaN normals; states {np.bincount(res['state'].ravel(), minlength=6)}")
        assert res.size == 80 and share >= 0.9
        assert sum(len(t) for t in tgt) < 0.75 * concat
        assert all(flat(t) for t in tgt)                                            # recomputed normals, whatever the poses
        layers = pv.z_layers(frames, maps, S["stride"], leaf)
        assert 1 in layers and 2 in layers and max(layers) >= 3                     # unions of one, two and many z layers
    assert sum(int(np.isnan(t[:, 4]).sum()) for t in pv.seeded_targets(1.0)) > 0    # the lone-voxel branch is in the list
    for leaf, radius in pv.ODD_PAIRS:
        assert radius < leaf or (radius / leaf) % 1 != 0


def test_leaf_zero_and_the_overflow_branch_are_the_concatenation():
    S = pv.seeded_list()
    c = cc.target(S["frames"], S["maps"].entries(5), S["stride"])
    assert pv.thin(c, 0.0)[0].tobytes() == c.tobytes()
    rows, overflow = pv.thin(c, 1e-6)
    assert overflow and rows.tobytes() == c.tobytes()
    rows, overflow = pv.thin(c, 0.2)
    assert not overflow and 0 < len(rows) < len(c)


# ---- the entry-order pair ---------------------------------------------------------------------------------------------------------------
def test_the_entry_order_pair_differs_in_a_centroid_and_nowhere_else():
    a, b, c = pv.ORDER_XS
    s0, s1 = pv.order_sums()
    assert all(0 <= float(x) < pv.ORDER_LEAF for x in (a, b, c))                    # one voxel
    assert s0 != s1 and abs(float(s0) - float(s1)) < 1e-6                           # (a + b) + c against (c + b) + a, in float32
    assert F32(s0 / F32(3)) != F32(s1 / F32(3))
    frames, maps, m = pv.order_pair()
    t0, t1 = (pv.target(frames, maps.entries(g), 300, pv.ORDER_LEAF) for g in (0, 1))
    assert len(t0) == len(t1) and t0.tobytes() != t1.tobytes()
    differ = np.flatnonzero((t0.view(np.uint32) != t1.view(np.uint32)).any(axis=1))
    assert (t0[differ, 0] != t1[differ, 0]).any()                                   # a centroid's x
    v0 = t0[np.flatnonzero(t0[:, 0] != t1[:, 0])]
    assert len(v0) == 1 and 0 <= v0[0, 0] < 1 and 0 <= v0[0, 1] < 1                 # the voxel of the three points, alone
    c0, c1 = (np.sort(cc.target(frames, maps.entries(g), 300).view(np.uint32).reshape(-1, 12), axis=0) for g in (0, 1))
    assert c0.tobytes() == c1.tobytes()                                             # the same union
    res, _ = pv.expected(frames, maps, m, pv.ORDER_LEAF, stride=300, threads=2)
    assert (res["state"][:, 0] != bev_amd.ICP_NO_CORRESPONDENCES).all()
