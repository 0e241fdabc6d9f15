"""CPU: scan-to-map coarse ICP without a GPU — the entry point in the library and the binding, the tool and its
argument checks, the checker's move of PointNormal records (submap_coarse_cases.py) against the oracle's transform, the
condition the seeded list puts on its inputs, and the checker composition on the coarse mirror tie, which must depend on the
entry order.  (The host plan is §6k's with a byte model of its own behind a defaulted parameter: tests/submapregcheck, run by
test_submap_registration_cpu.py, pins that every existing call plans as before.)"""
import ctypes as C
import subprocess

import numpy as np

import bev_amd
import icp_lib
import oracle_lib as orc
import reg_cases as rc
import submap_coarse_cases as cc
import submap_reg_cases as sc

CLI = bev_amd.PKG_DIR / "host" / "batch_submap_top_part_registration"
INVALID = -1
F32 = np.float32


def test_entry_point_is_exported_and_bound_and_refuses_a_null_context():
    lib = bev_amd.load_lib()
    name = "bev_submap_coarse_registration_device_resident"
    assert name in bev_amd.ABI_SYMBOLS and hasattr(lib, name)
    assert hasattr(bev_amd.BevContext, "submap_coarse_registration_device")
    assert lib.bev_abi_version() == 1                      # the change only adds
    assert bev_amd.SUBMAP_COARSE_MAX_TARGET == cc.COARSE_MAX_TARGET
    header = (bev_amd.REPO_DIR / "include" / "bev_mi355x.h").read_text()
    assert "#define BEV_SUBMAP_COARSE_MAX_TARGET (1u << 22)" in header and f"int {name}(" in header
    moffs = np.array([0, 1], dtype=np.uint64)
    eframe = np.zeros(1, dtype=np.int32)
    epose = sc.IDENTITY.reshape(1, 12).copy()
    pn = np.zeros((4, 12), F32)
    counts = np.array([4], np.uint32)
    m = sc.matches([(0, 0, 0.0)])
    out = np.full(2 * bev_amd.ICP_RESULT_DTYPE.itemsize, 0xA5, dtype=np.uint8)
    best = np.full(1, 0x5A5A5A5A, dtype=np.int32)
    assert lib.bev_submap_coarse_registration_device_resident(
        None, 1, pn.ctypes.data, 4, counts.ctypes.data, 1, moffs.ctypes.data_as(C.POINTER(C.c_uint64)), eframe.ctypes.data,
        epose.ctypes.data, 1, m.ctypes.data, None, out.ctypes.data, best.ctypes.data) == INVALID
    assert (out == 0xA5).all() and best[0] == 0x5A5A5A5A


def _run(*args, cwd=None):
    return subprocess.run([str(CLI), *[str(a) for a in args]], capture_output=True, text=True, timeout=60, cwd=cwd)


def test_tool_exists_and_refuses_wrong_arguments_before_it_creates_a_context(tmp_path):
    assert CLI.exists(), "host CLI not built"
    for args in ((), ("m.txt",), ("m.txt", "/nowhere")):
        r = _run(*args, cwd=tmp_path)
        assert r.returncode == 1 and r.stderr.startswith("Usage: batch_submap_top_part_registration <match_result_text_file> "), args
    (tmp_path / "non_ground_point_cloud").mkdir()
    (tmp_path / "m.txt").write_text("0 0 0.0\n")
    for window in ("-1", "two", "2x", ""):
        r = _run(tmp_path / "m.txt", tmp_path, window, cwd=tmp_path)
        assert r.returncode == 1 and f"half_window '{window}': expected an integer >= 0" in r.stderr, (window, r.stderr)
    r = _run(tmp_path / "m.txt", tmp_path, 2, 5, cwd=tmp_path)
    assert r.returncode == 1 and "chunk '5': expected an integer >= 2 * half_window + 2" in r.stderr
    for leaf in ("-0.5", "nan", "inf", "0.2x", ""):
        r = _run(tmp_path / "m.txt", tmp_path, 1, 8, leaf, cwd=tmp_path)
        assert r.returncode == 1 and "expected a finite number >= 0" in r.stderr and "Usage: batch_submap_top_part_registration" in r.stderr, leaf
    r = _run(tmp_path / "m.txt", tmp_path, 1, cwd=tmp_path)                    # no pose file
    assert r.returncode == 1 and "keyframe_pose.csv" in r.stderr
    (tmp_path / "keyframe_pose.csv").write_text(",".join(["0", "1.0", "2.0", "0.0", "0", "0", "0", "1", "0", "0", "0", "1", "0", "0", "0", "1"]) + "\n")
    (tmp_path / "m.txt").write_text("0 3 0.0\n")
    r = _run(tmp_path / "m.txt", tmp_path, 1, cwd=tmp_path)                    # an index outside the (zero) clouds
    assert r.returncode == 1 and "outside the 0 clouds" in r.stderr
    assert "bev_create" not in r.stderr and "HIP" not in r.stderr


def test_the_checkers_move_equals_the_oracles_transform_on_the_positions():
    rng = np.random.default_rng(77)
    pn = cc.frame(700, 31)
    pn[::50, 0] = np.nan
    pn[7::90, 1] = np.inf
    pn[3::70, 4:7] = np.nan
    pn[11] = [1e30, -1e30, 3e38, 0, 1, 0, 0, 0, 0.5, 0, 0, 0]
    cloud = rc.points(pn[:, :3])
    mats = [sc.IDENTITY, sc.shift(0.5, -0.25, 3.0), sc.planar(33.0, 4.0, -7.0), cc.pose3d(2.0, -3.0, 40.0, 1.0, 2.0, -0.5),
            np.array([1e38, 0, 0, 0, 0, 1e38, 0, 0, 0, 0, 1, 0], F32),                      # overflows to infinity
            (rng.uniform(-2, 2, 12)).astype(F32)]                                           # no rotation
    for m in mats:
        got = cc.move(pn, m)
        exp = orc.transform_cloud(cloud, m)
        for k, name in enumerate("xyz"):
            g, e = got[:, k], np.ascontiguousarray(exp[name])
            same = (g.view(np.uint32) == e.view(np.uint32)) | (np.isnan(g) & np.isnan(e))   # (the oracle's NaNs keep their payload)
            assert same.all(), (name, m, int((~same).sum()))
        assert (got.view(np.uint32)[np.isnan(got)] == 0x7FC00000).all()
        assert not got[:, [3, 7, 9, 10, 11]].any() and np.array_equal(got[:, 8], pn[:, 8])
        # the normal: the same association without the translation, neither renormalised nor flipped
        M = np.asarray(m, F32).reshape(3, 4)
        with np.errstate(all="ignore"):
            n0 = M[0, 0] * pn[:, 4] + (M[0, 1] * pn[:, 5] + M[0, 2] * pn[:, 6])
        ok = ~np.isnan(n0)
        assert np.array_equal(got[ok, 4], n0[ok]) and np.isnan(got[~ok, 4]).all()
    # under a planar rotation a unit normal stays one; under the matrix that is no rotation it does not, and is left so
    assert np.allclose(np.linalg.norm(cc.move(cc.frame(50, 1), mats[2])[:, 4:7], axis=1), 1.0, atol=1e-6)
    assert not np.allclose(np.linalg.norm(cc.move(cc.frame(50, 1), mats[5])[:, 4:7], axis=1), 1.0, atol=1e-3)
    # the concatenation is in entry order and cuts every frame at the stride
    a, b = cc.frame(30, 2), cc.frame(20, 3)
    t = cc.target([a, b], [(1, sc.IDENTITY), (0, sc.shift(1.0)), (1, sc.shift(-1.0))], stride=25)
    assert len(t) == 20 + 25 + 20 and t[:20].tobytes() == cc.move(b, sc.IDENTITY).tobytes()
    assert t[20:45].tobytes() == cc.move(a[:25], sc.shift(1.0)).tobytes()


def test_the_seeded_list_meets_its_condition_on_the_checker():
    icp_lib.build()
    S = cc.seeded_list()
    m, H = S["m"], S["H"]
    res, best = cc.seeded_expected()
    share = cc.condition_share(res)
    print(f"{len(m)} matches, {len(S['maps'])} maps: {share:.3f} keep correspondences for two iterations or more under both guesses; "
          f"states {np.bincount(res['state'].ravel(), minlength=6)}, best {np.bincount(best, minlength=2)}")
    assert share >= 0.9
    assert 900 <= len(m) <= 1100 and (m["match_idx"][: S["n_id"]] < 2 * H).all() and S["n_id"] >= 0.4 * len(m)
    sizes = [len(f) for f in S["frames"]]
    assert min(sizes) == 0 and max(sizes) == 512 and max(sizes) > S["stride"]
    n_ent = [len(S["maps"].entries(g)) for g in range(2 * H, 3 * H)]
    assert min(n_ent) == 1 and max(n_ent) == 6
    poses = np.array([p for g in range(2 * H, 3 * H) for _, p in S["maps"].entries(g)]).reshape(-1, 3, 4)
    assert (np.abs(poses[:, 2, 0]) > 1e-3).any() and (np.abs(poses[:, 2, 1]) > 1e-3).any()   # pitch and roll occur
    assert (poses[:, 2, 0] == 0).any()                                                       # and planar poses
    assert (best == 0).any() and (best == 1).any()


def test_the_checker_composition_depends_on_the_entry_order_of_the_coarse_mirror_tie():
    icp_lib.build()
    frames, maps, m = cc.mirror_tie()
    a, src = frames
    assert (a[:, 4] != 0).all() and np.allclose(np.linalg.norm(a[:, 4:7], axis=1), 1.0, atol=1e-6) and (a[:, 2] == a[0, 2]).all()
    t0, t1 = cc.target(frames, maps.entries(0)), cc.target(frames, maps.entries(1))
    assert len(t0) == 800 and t0[:400].tobytes() == t1[400:].tobytes() and t0[400:].tobytes() == t1[:400].tobytes()
    # the tie itself: every source point is exactly as far from both images of its own point, and nothing is nearer
    i0, d0 = icp_lib.nn(t0, src)
    i1, d1 = icp_lib.nn(t1, src)
    assert (i0 < 400).all() and (i1 < 400).all() and d0.tobytes() == d1.tobytes()
    assert (d0 == F32(0.25 + 1.0 / 64.0)).all()
    assert (t0[i0, 0] - src[:, 0] == F32(0.5)).all() and (t1[i1, 0] - src[:, 0] == F32(-0.5)).all()
    # the corresponding target changes d = n . (t - s): +0.5 nx - 0.125 ny against -0.5 nx - 0.125 ny
    d = lambda t, i: (t[i, 4:7] * (t[i, :3] - src[:, :3])).sum(axis=1)
    assert np.array_equal(t0[i0, 4:7], t1[i1, 4:7]) and (d(t0, i0) != d(t1, i1)).all()
    res, best = cc.expected(frames, maps, m, threads=2)
    assert (res["state"] != bev_amd.ICP_NO_CORRESPONDENCES).all()
    assert res[0, 0].tobytes() != res[1, 0].tobytes()      # guess 0 starts on the tie (guess 1 turns the source by 180 degrees: no tie)
