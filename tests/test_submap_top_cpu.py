"""CPU: the top part over the union of a map's moved full clouds as the coarse stage's target without a GPU —
the three functions in the library and the bindings; the tool's BEV_SUBMAP_TOP_UNION and each of its refusals;
bev_submap_top_part_max_out; the host plan with its byte model, by the stand-alone tests/submaptopcheck, plain and as a second
program under the address and undefined-behaviour sanitizers; the condition the seeded list puts on its inputs, on the
checker's results alone; and the checker on the edge clouds, so their expected rows are known before a GPU sees them."""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import bev_amd
import icp_lib
import regfront_lib as rf
import submap_reg_cases as sc
import submap_top_cases as tc

DIR = Path(__file__).resolve().parent / "submaptopcheck"
TOP = bev_amd.PKG_DIR / "host" / "batch_submap_top_part_registration"
WHOLE = bev_amd.PKG_DIR / "host" / "batch_submap_registration"
INVALID = -1
F32 = np.float32
SANITIZE = "-fsanitize=address,undefined -fno-omit-frame-pointer"
NEW = ("bev_submap_top_part_cloud_device_resident", "bev_submap_top_part_coarse_registration_device_resident",
       "bev_submap_top_part_max_out")
VARS = ("BEV_SUBMAP_PN_LEAF", "BEV_SUBMAP_TOP_UNION")


@pytest.fixture(scope="module", autouse=True)
def _checkers():
    icp_lib.build()
    rf.build()


# ---- exports, bindings ------------------------------------------------------------------------------------------------------------
def test_the_three_functions_are_exported_and_bound_and_refuse_a_null_context():
    lib = bev_amd.load_lib()
    assert set(NEW) <= set(bev_amd.ABI_SYMBOLS) and all(hasattr(lib, n) for n in NEW)
    for name in ("submap_top_part_cloud_device", "submap_top_part_coarse_registration_device"):
        assert hasattr(bev_amd.BevContext, name), name
    assert lib.bev_abi_version() == 1                      # the change only adds
    header = (bev_amd.REPO_DIR / "include" / "bev_mi355x.h").read_text()
    assert all(f"int {n}(" in header for n in NEW[:2]) and f"size_t {NEW[2]}(" in header
    assert "#define BEV_SUBMAP_TOP_MAX_UNION (1u << 24)" in header
    moffs = np.array([0, 1], dtype=np.uint64)
    offs = np.array([0, 4], dtype=np.uint64)
    eframe = np.zeros(1, dtype=np.int32)
    epose = sc.IDENTITY.reshape(1, 12).copy()
    cloud = tc.column(np.arange(4))
    pn = np.zeros((4, 12), F32)
    counts = np.array([4], np.uint32)
    m = sc.matches([(0, 0, 0.0)])
    out = np.full(2 * bev_amd.ICP_RESULT_DTYPE.itemsize, 0xA5, dtype=np.uint8)
    best = np.full(1, 0x5A5A5A5A, dtype=np.int32)
    rows, n_rows = np.full(51 * 48, 0xA5, dtype=np.uint8), np.full(4, 0xA5, dtype=np.uint8)
    u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    assert lib.bev_submap_top_part_coarse_registration_device_resident(
        None, 1, cloud.ctypes.data, u64(offs), pn.ctypes.data, 4, counts.ctypes.data, 0.2, 2.0, None, 1, u64(moffs),
        eframe.ctypes.data, epose.ctypes.data, 1, m.ctypes.data, None, out.ctypes.data, best.ctypes.data) == INVALID
    assert lib.bev_submap_top_part_cloud_device_resident(
        None, 1, cloud.ctypes.data, u64(offs), 0.2, 2.0, None, 1, u64(moffs), eframe.ctypes.data, epose.ctypes.data, 51,
        rows.ctypes.data, n_rows.ctypes.data) == INVALID
    assert (out == 0xA5).all() and best[0] == 0x5A5A5A5A and (rows == 0xA5).all() and (n_rows == 0xA5).all()


def test_max_out_is_the_front_ends_bound_of_the_union():
    for n in (0, 1, 4, 5, 19, 20, 99, 100, 20475, 70001, 2_800_000, tc.MAX_UNION):
        assert bev_amd.submap_top_part_max_out(n) == tc.max_out(n) == bev_amd.regfront_max_out(n), n
    assert tc.max_out(tc.MAX_UNION) < 1 << 22               # the selection's sort stays within §6l's size
    # the bound holds where it is tight: 100 cells of 22 records each emit round(4.4) = 4: 400 <= 2200 / 5 + 51; cells of 23: 5
    assert 100 * 5 <= tc.max_out(100 * 23)


# ---- the tool's variable ------------------------------------------------------------------------------------------------------------
def _run(tool, *args, cwd=None, **env_vars):
    env = {k: v for k, v in os.environ.items() if k not in VARS}
    env.update({k: v for k, v in env_vars.items() if v is not None})
    return subprocess.run([str(tool), *[str(a) for a in args]], capture_output=True, text=True, timeout=60, cwd=cwd, env=env)


def _no_gpu_work(r, tmp_path):
    assert r.returncode == 1 and r.stdout == "", r.stdout
    assert "bev_create" not in r.stderr and "HIP" not in r.stderr and "keyframe_pose.csv" not in r.stderr, r.stderr
    assert len(r.stderr.strip().splitlines()) == 1, r.stderr
    assert not (tmp_path / "icp_precision_report.txt").exists()                     # refused before anything is created


def test_the_tool_reads_its_variable_and_refuses_before_any_gpu_work(tmp_path):
    assert TOP.exists() and WHOLE.exists(), "host CLI not built"
    (tmp_path / "non_ground_point_cloud").mkdir()
    (tmp_path / "m.txt").write_text("0 0 0.0\n")
    args = (tmp_path / "m.txt", tmp_path, 1)
    for text in ("2", "yes", "-1", "1.0", "01", " 1", "true"):                      # neither 0 nor 1
        r = _run(TOP, *args, cwd=tmp_path, BEV_SUBMAP_TOP_UNION=text, BEV_SUBMAP_PN_LEAF="0.5")
        _no_gpu_work(r, tmp_path)
        assert f"BEV_SUBMAP_TOP_UNION '{text}': expected 0 or 1" in r.stderr, (text, r.stderr)
    for leaf in (None, "", "0", "0.0"):                                             # 1 without a leaf: one line naming both
        r = _run(TOP, *args, cwd=tmp_path, BEV_SUBMAP_TOP_UNION="1", BEV_SUBMAP_PN_LEAF=leaf)
        _no_gpu_work(r, tmp_path)
        assert "BEV_SUBMAP_TOP_UNION" in r.stderr and "BEV_SUBMAP_PN_LEAF" in r.stderr, (leaf, r.stderr)
    r = _run(TOP, *args, cwd=tmp_path, BEV_SUBMAP_TOP_UNION="1", BEV_SUBMAP_PN_LEAF="nan")   # the leaf's own refusal comes first
    _no_gpu_work(r, tmp_path)
    assert "BEV_SUBMAP_PN_LEAF 'nan': expected a finite number >= 0" in r.stderr
    for union, leaf in ((None, None), ("", None), ("0", None), ("0", "0.5"), ("1", "0.5"), ("1", "1e-3")):
        r = _run(TOP, *args, cwd=tmp_path, BEV_SUBMAP_TOP_UNION=union, BEV_SUBMAP_PN_LEAF=leaf)   # accepted: the pose file is next
        assert r.returncode == 1 and "BEV_SUBMAP_TOP_UNION" not in r.stderr and "keyframe_pose.csv" in r.stderr, (union, leaf, r.stderr)
    r = _run(TOP, cwd=tmp_path, BEV_SUBMAP_TOP_UNION="1", BEV_SUBMAP_PN_LEAF="0.5")  # the usage line stays what it is
    assert r.returncode == 1 and r.stderr.startswith(
        "Usage: batch_submap_top_part_registration <match_result_text_file> <keyframes_root_dir> <half_window> [<chunk> [<map_leaf>]]")
    r = _run(WHOLE, *args, cwd=tmp_path, BEV_SUBMAP_TOP_UNION="maybe")              # no coarse stage: the variable is not read
    assert r.returncode == 1 and "BEV_SUBMAP_TOP_UNION" not in r.stderr and "keyframe_pose.csv" in r.stderr


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
    words = lines[-1].replace(",", "").split()   # ok: submaptopcheck: P plans T of them top-part-over-the-union plans G launch groups K of ...
    plans, top, groups, oversize = int(words[2]), int(words[4]), int(words[9]), int(words[12])
    assert plans == 2500 and top == 250 * 2 and groups > plans and 0 < oversize < groups


def test_the_plan_keeps_its_byte_models_and_existing_calls_plan_as_before():
    built, run = _build_and_run("submaptopcheck")
    assert built.returncode == 0, built.stdout
    _assert_ok(run)


def test_the_same_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    r = subprocess.run(["gcc", *SANITIZE.split(), "-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("the sanitizer runtime is not installed: " + (r.stderr.strip().splitlines() or ["gcc failed"])[-1])
    built, run = _build_and_run("submaptopcheck_san")      # a stand-alone host program, run directly
    assert built.returncode == 0, built.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr
    _assert_ok(run)


def test_the_checkers_group_count_restates_the_plans_byte_model():
    S = tc.seeded_list()
    used = list(range(len(S["maps"])))
    assert tc.map_bytes(2_800_000) == 8 * 2_800_000 + 28416 + 136 * 560051 + 8 * (1 << 20) + 16456
    n_groups, alone = tc.group_count(S["clouds"], S["maps"], used, 600000)
    assert n_groups >= 4 and 1 <= alone < len(S["maps"])
    assert tc.group_count(S["clouds"], S["maps"], used, 1 << 40) == (1, 0)


# ---- the seeded list --------------------------------------------------------------------------------------------------------------------
def test_the_seeded_list_meets_its_condition_on_the_checker():
    S = tc.seeded_list()
    clouds, maps, m, H = S["clouds"], S["maps"], S["m"], S["H"]
    sizes = [len(c) for c in clouds[:H]]
    assert H == 16 and len(clouds) == 32 and set(tc.LIST_SIZES) <= set(sizes) and 1500 <= min(sizes) and max(sizes) < 3500
    assert all((c["label"] == 0).any() and (c["label"] == 1).any() for c in clouds)
    assert sorted({len(maps.entries(g)) for g in range(len(maps))}) == [1, 2, 3, 4, 5, 6]
    assert len(m) == 2 * H                                                          # two guesses each: 64 problems
    tops = tc.seeded_tops()
    for g in range(len(maps)):
        assert 0 < len(tops[g]) <= tc.max_out(tc.union_cap(clouds, maps, g)) and (tops[g][:, 2] == 0).all()
    # the top part over the union is not the concatenation of the entries' own top parts: the union fills cells that no entry
    # fills alone, and ranks the records of all entries together
    per_sweep = [sum(len(rf.top_part(tc.union(clouds, [e]))) for e in maps.entries(g)) for g in range(len(maps))]
    assert any(len(tops[g]) != per_sweep[g] for g in range(len(maps)) if len(maps.entries(g)) > 1)
    for leaf, radius in [(l, tc.RADIUS) for l in tc.LEAVES] + [tc.ODD_PAIR]:
        res, best = tc.seeded_expected(leaf, radius)
        tgt = tc.seeded_targets(leaf, radius)
        ok = tc.condition(res)
        print(f"leaf {leaf} radius {radius}: {int(ok.sum())} of {res.size} problems keep correspondences for two iterations or more; "
              f"{sum(len(t) for t in tops)} rows thinned to {sum(len(t) for t in tgt)}; states {np.bincount(res['state'].ravel(), minlength=6)}")
        assert res.size == 64 and ok.all()                                          # every problem, no share left out
        assert all(len(t) > 0 for t in tgt)                                         # every map has a target
        assert all(((t[:, 6] == 0) | np.isnan(t[:, 4])).all() and (t[:, 2] == 0).all() for t in tgt)
    assert tc.ODD_PAIR[1] < tc.ODD_PAIR[0]


def test_leaf_zero_is_the_top_part_and_the_overflow_branch_keeps_it_with_normals():
    t = tc.seeded_tops()[5]
    assert tc.thin(t, 0.0)[0].tobytes() == tc.rows_of_top(t).tobytes()
    rows, overflow = tc.thin(t, 1e-6)
    assert overflow and rows[:, :3].tobytes() == t[:, :3].tobytes() and (rows[:, 4:6] != 0).any()
    rows, overflow = tc.thin(t, 0.2)
    assert not overflow and 0 < len(rows) < len(t)


# ---- the edge clouds ----------------------------------------------------------------------------------------------------------------------
def test_the_checker_on_the_edge_clouds():
    E = {name: tc.edge_expected(name) for name in tc.edge_cases()}
    n = {name: [len(r) for r in rows] for name, rows in E.items()}
    print(n)
    assert n["cell_counts_19_20"] == [0, 4, 0]                  # 19: skipped; 10 + 10: kept by the union alone; 10: skipped
    assert n["rank_rounding"] == [4, 5, 5, 6]                   # 22, 23, 27, 28 records
    assert n["threshold_in_tie_run"] == [6] and n["empty_targets"] == [0, 0]
    # the tie rule: where every z is tied the selection is the first entry's first records, so swapping the entries gives the
    # other rows; where each z is tied once across the entries, the earlier entry's record comes first of the two
    clouds, maps = tc.edge_cases()["tie_rule"]
    twice, ab, ba, cd, dc = E["tie_rule"]
    assert np.array_equal(twice[:, 0], clouds[0]["x"][:16]) and twice.tobytes() == ab.tobytes()
    assert np.array_equal(ba[:, 0], clouds[1]["x"][:16]) and (ba[:, 0] >= 5).all()
    assert len(cd) == len(dc) == 16 and (cd[0::2, 0] < 1).all() and (cd[1::2, 0] >= 5).all()
    assert (dc[0::2, 0] >= 5).all() and (dc[1::2, 0] < 1).all()
    # the threshold inside the run of equal z: the four higher records, then the run's two lowest union indices
    clouds, maps = tc.edge_cases()["threshold_in_tie_run"]
    run = np.flatnonzero(clouds[0]["z"] == 5.0)[:2]
    assert np.array_equal(E["threshold_in_tie_run"][0][4:, 0], clouds[0]["x"][run])
    # -0 and +0 are one value: the selection is by index alone; the same cloud again under a zero shift changes nothing
    clouds, maps = tc.edge_cases()["degenerate_digits"]
    assert np.array_equal(E["degenerate_digits"][2][:, 0], clouds[2]["x"][:6])
    assert np.array_equal(E["degenerate_digits"][0][:, 0], clouds[0]["x"][:10])     # all one z: the first ten records
    assert np.array_equal(E["degenerate_digits"][1][:, 0], clouds[1]["x"][np.argsort(-clouds[1]["z"], kind="stable")[:5]])   # one ulp apart
    # poses: moved out, moved in, the edge cells, the overflowing matrix, the roll that reverses the order
    p = n["poses"]
    assert p[0] == 0 and p[1] == 12 and p[2] == 24 and p[4] == 12
    base_top, rolled = E["poses"][5], E["poses"][6]
    assert len(base_top) == len(rolled) == 24 and (base_top[:, 0] < 1).all() and (rolled[:, 0] >= 3).all()
    assert n["labels_and_non_finite"] == [13]
