"""CPU: scan-to-map registration against maps thinned by a voxel grid over their union without a GPU — the
sort schedule (csrc/bev_submap_vox_plan.h) executed on the host and the plan at the union grid's sizes, by the stand-alone
tests/submapvoxcheck, plain and as a second program under the address and undefined-behaviour sanitizers; the three entry
points in the library and the bindings; the tool's <map_leaf> argument; the conditions on the inputs of the main GPU case,
so that it cannot pass vacuously; and the checker composition (submap_vox_cases.py) on the mirror-tie maps, which must no
longer depend on the entry order once every voxel of the union holds one point."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import bev_amd
import fineicp_lib as fl
import submap_reg_cases as sc
import submap_vox_cases as vc

DIR = Path(__file__).resolve().parent / "submapvoxcheck"
CLI = bev_amd.PKG_DIR / "host" / "batch_submap_registration"
INVALID = -1
SANITIZE = "-fsanitize=address,undefined -fno-omit-frame-pointer"
NEW = ("bev_submap_voxel_registration_device_resident", "bev_submap_voxel_registration_batch",
       "bev_submap_voxel_cloud_device_resident")


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
    assert [l for l in lines if l.startswith("ok:")] == lines[-1:], run.stdout
    assert "VOX" not in run.stdout
    words = lines[-1].replace(",", "").split()      # ok: submapvoxcheck: tile T, S sorts in L launches, P plans, G launch groups, K of ...
    assert words[:3] == ["ok:", "submapvoxcheck:", "tile"] and int(words[3]) == vc.TILE, lines[-1]
    sorts, launches, plans, groups, oversize = int(words[4]), int(words[7]), int(words[9]), int(words[11]), int(words[14])
    assert sorts == 30 and launches > 10 * sorts          # ten sizes, alone and beside larger maps; stages across tiles ran
    assert plans == 400 and groups > plans and 0 < oversize < groups


def test_the_sort_schedule_sorts_and_the_plan_keeps_its_invariants_at_the_larger_size():
    built, run = _build_and_run("submapvoxcheck")
    assert built.returncode == 0, built.stdout
    _assert_ok(run)


def test_the_same_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    r = subprocess.run(["gcc", *SANITIZE.split(), "-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("the sanitizer runtime is not installed: " + (r.stderr.strip().splitlines() or ["gcc failed"])[-1])
    built, run = _build_and_run("submapvoxcheck_san")      # a stand-alone host program, run directly
    assert built.returncode == 0, built.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr
    _assert_ok(run)


def test_the_three_entry_points_are_exported_and_refuse_a_null_context():
    lib = bev_amd.load_lib()
    assert set(NEW) <= set(bev_amd.ABI_SYMBOLS) and all(hasattr(lib, n) for n in NEW)
    for name in ("submap_voxel_registration_device", "submap_voxel_registration_batch", "submap_voxel_cloud_device"):
        assert hasattr(bev_amd.BevContext, name), name
    assert lib.bev_abi_version() == 1                      # the change only adds
    offs = np.array([0, 4], dtype=np.uint64)
    moffs = np.array([0, 1], dtype=np.uint64)
    eframe = np.zeros(1, dtype=np.int32)
    epose = sc.IDENTITY.reshape(1, 12).copy()
    buf = np.zeros(4, dtype=bev_amd.POINT_DTYPE)
    m = sc.matches([(0, 0, 0.0)])
    out = np.full(bev_amd.ICP_RESULT_DTYPE.itemsize, 0xA5, dtype=np.uint8)
    rows, counts = np.full(16, 0xA5, dtype=np.uint8), np.full(4, 0xA5, dtype=np.uint8)
    u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    assert lib.bev_submap_voxel_registration_device_resident(None, 1, buf.ctypes.data, u64(offs), 0.2, 0.2, 1, u64(moffs),
                                                             eframe.ctypes.data, epose.ctypes.data, 1, m.ctypes.data, None, None,
                                                             None, out.ctypes.data) == INVALID
    VP = C.c_void_p * 1
    n = (C.c_uint32 * 1)(4)
    assert lib.bev_submap_voxel_registration_batch(None, 1, VP(buf.ctypes.data), n, 0.2, 0.2, 1, u64(moffs), eframe.ctypes.data,
                                                   epose.ctypes.data, 1, m.ctypes.data, None, out.ctypes.data) == INVALID
    assert lib.bev_submap_voxel_cloud_device_resident(None, 1, buf.ctypes.data, u64(offs), 0.2, 0.2, 1, u64(moffs),
                                                      eframe.ctypes.data, epose.ctypes.data, 4, rows.ctypes.data,
                                                      counts.ctypes.data) == INVALID
    assert (out == 0xA5).all() and (rows == 0xA5).all() and (counts == 0xA5).all()


def _run(*args, cwd=None):
    return subprocess.run([str(CLI), *[str(a) for a in args]], capture_output=True, text=True, timeout=60, cwd=cwd)


def test_the_tool_refuses_a_bad_map_leaf_with_the_usage_line(tmp_path):
    assert CLI.exists(), "host CLI not built"
    (tmp_path / "non_ground_point_cloud").mkdir()
    (tmp_path / "m.txt").write_text("0 0 0.0\n")
    for leaf in ("-0.2", "-1", "nan", "inf", "-inf", "0.2x", "leaf", "", "1e99"):
        r = _run(tmp_path / "m.txt", tmp_path, 1, 256, leaf, cwd=tmp_path)
        assert r.returncode == 1 and f"map_leaf '{leaf}': expected a finite number >= 0" in r.stderr, (leaf, r.stderr)
        assert "Usage: batch_submap_registration <match_result_text_file> <keyframes_root_dir> <half_window> [<chunk> [<map_leaf>]]" in r.stderr
        assert not (tmp_path / "icp_precision_report_submap.txt").exists()          # refused before anything is created
    for leaf in ("0", "0.0", "0.2", "1e-3"):                                        # accepted: the next complaint is the pose file's
        r = _run(tmp_path / "m.txt", tmp_path, 1, 256, leaf, cwd=tmp_path)
        assert r.returncode == 1 and "map_leaf" not in r.stderr and "keyframe_pose.csv" in r.stderr, (leaf, r.stderr)
    assert "bev_create" not in r.stderr and "HIP" not in r.stderr


def test_the_main_case_loses_points_to_the_union_grid_and_mixes_entries_in_a_voxel():
    """The conditions on the inputs of the main GPU case, asserted by the checker alone: at both leaves every map of two or
    more entries loses at least a quarter of its concatenation's points to the union grid and holds at least one voxel of
    three or more points that come from two or more entries."""
    fl.build()
    S = vc.main_case()
    maps, multi = S["maps"], S["multi"]
    assert len(multi) >= 20 and {len(maps.entries(g)) for g in range(len(maps))} == set(range(0, 9))
    assert set(multi) <= set(S["m"]["match_idx"].tolist())
    vox = vc.voxel_clouds(S["clouds"], {f for g in multi for f, _ in maps.entries(g)})
    for leaf in vc.MAP_LEAVES:
        tg = vc.targets(S["clouds"], maps, multi, leaf, vox=vox)
        for g in multi:
            concat, thin = tg[g]
            n_vox, mixed = vc.union_voxels(concat, vc.entry_index(vox, maps.entries(g)), leaf)
            assert n_vox == len(thin), (g, leaf, n_vox, len(thin))         # (the restated grid counts what the checker counts)
            assert 4 * len(thin) <= 3 * len(concat), f"map {g} at {leaf}: {len(concat)} -> {len(thin)} points"
            assert mixed >= 3, f"map {g} at {leaf}: no voxel of three points from two entries"


def test_the_mirror_tie_no_longer_follows_the_entry_order_once_the_union_is_thinned():
    fl.build()
    clouds, maps, m = sc.mirror_tie()
    vox = vc.voxel_clouds(clouds, [0])
    tg = vc.targets(clouds, maps, [0, 1], 0.2, vox=vox)
    assert len(tg[0][1]) == len(tg[0][0]) == 2 * len(vox[0])              # one point per voxel of the union
    assert tg[0][0].tobytes() != tg[1][0].tobytes() and vc.rows(tg[0][1]).tobytes() == vc.rows(tg[1][1]).tobytes()
    for prm in (fl.params(**fl.WHOLE), fl.params(**fl.FINE)):
        thin = vc.expected(clouds, maps, m, prm, 0.2, threads=2)
        assert thin[0]["state"] != bev_amd.ICP_NO_CORRESPONDENCES
        assert thin[0].tobytes() == thin[1].tobytes()                      # the order of entries no longer decides
        plain = vc.expected(clouds, maps, m, prm, 0.0, threads=2)
        assert plain.tobytes() == sc.expected(clouds, maps, m, prm, threads=2).tobytes()
        assert plain[0].tobytes() != plain[1].tobytes()                    # as it does without the second grid
