"""CPU: the seeded inputs of tests/reg_cases.py against plain references, and proof on the host that they reach what
test_registration_batch_gpu.py needs them for — the checkers' nearest neighbour on the skewed geometries equals a numpy
brute force, the front end's chain checker equals its three stages at every (leaf, radius), and the ragged pack crosses
the fine stage's voxel groups and launches with every named frame visible in a compared result."""
import os

import numpy as np
import pytest

import bev_amd
import fineicp_lib as fl
import icp_lib as il
import reg_cases as rc
import regfront_lib as rl

THREADS = min(16, os.cpu_count() or 4)
F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _checker():
    fl.build()
    il.build()
    rl.build()


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("D", [0.7, 1.0, 4.0, 10.0])
def test_nearest_neighbour_on_skewed_geometry_equals_brute_force(D):
    rng = np.random.default_rng(31)
    grids = set()
    for name, tgt in rc.skewed_targets():
        assert tgt.shape == (rc.SKEW_N, 3) and tgt.dtype == F32
        for kind in rc.SOURCE_KINDS:
            src = rc.skewed_source(name, tgt, kind, D)
            if kind == "outside":  # wholly outside the target's box, by less than D (at 1e6 a float step is 1 / 16: on it)
                assert (src[:, 0] >= tgt[:, 0].max()).all() and (src[:, 0] - tgt[:, 0].max() < D).all(), name
                assert name == "outlier" or (src[:, 0] > tgt[:, 0].max()).all(), name
            q = src[rng.permutation(len(src))[:200]]
            idx, dist = rc.brute_nn(tgt, q)
            for lib, qq, tt in ((fl, q, tgt), (il, rc.point_normals(q, 1), rc.point_normals(tgt, 2))):
                gi, gd = lib.nn(tt, qq)
                assert np.array_equal(gi, idx) and _same(gd, dist), f"{name} {kind} {lib.__name__}"
    # what the geometries are for, from the grid's own arithmetic (reg_grid_build, restated in float32)
    for name, tgt in rc.skewed_targets():
        ex, ey = F32(tgt[:, 0].max() - tgt[:, 0].min()), F32(tgt[:, 1].max() - tgt[:, 1].min())
        dim = int(np.ceil(np.sqrt(F32(len(tgt)))))
        with np.errstate(all="ignore"):
            s = np.maximum(ex, ey) / F32(dim)
            ok = s > 0 and np.isfinite(s) and np.isfinite(F32(1) / s)
        if not ok:
            grids.add((name, "one cell"))
        elif int(ey * (F32(1) / s)) + 1 == 1:
            grids.add((name, "ny == 1"))
        if name == "outlier":  # every point but the outlier within one cell of the corner
            assert ((tgt[:, 0] - tgt[:, 0].min()) / s < 1).sum() == len(tgt) - 1
    assert {("vertical_line", "one cell"), ("identical", "one cell"), ("subnormal_extent", "one cell"),
            ("strip", "ny == 1")} <= grids, grids
    sub = dict(rc.skewed_targets())["subnormal_extent"]
    assert 0 < sub[:, 0].max() < np.finfo(F32).tiny  # subnormal, not flushed by the host
    lat = dict(rc.skewed_targets())["lattice"]
    _, d = rc.brute_nn(lat, rc.skewed_source("lattice", lat, "near", 1.0)[:2:2])
    assert d[0] == F32(0.25)  # half a step from two lattice points: a tie


def test_chain_checker_equals_its_stages_at_every_leaf_and_radius():
    cloud = np.concatenate([rc.scene(40000, 1), rc.moved(rc.scene(20000, 2), 30.0, 25.0, -40.0)])
    cloud["x"][::1000] = np.nan
    seen = set()
    for (leaf, radius), vp in [(lr, (0.0, 0.0, 0.0)) for lr in rc.LEAF_RADIUS] + [((0.35, 3.3), (5.0, -3.0, 0.0))]:
        got = rl.chain(cloud, leaf, radius, vp)
        flat = rl.top_part(cloud)
        vox, info = rl.voxel(flat, leaf, want_info=True)
        nrm, nn = rl.normals(vox, radius, vp, want_nn=True)
        exp = np.zeros((len(vox), 12), F32)
        exp[:, :4] = vox
        exp[:, 4:8] = nrm[:, :4]
        exp[:, 8] = nrm[:, 4]
        assert _same(got, exp), (leaf, radius)
        seen |= {(min(int(k), 3)) for k in np.unique(nn)}
        if leaf == 1e-6:
            assert info[0] == 1 and _same(vox, flat)  # the overflow branch: the input unchanged
        if leaf == 500.0:  # the four voxels around the origin; one voxel for a frame in one quadrant
            assert len(vox) <= 4 and len(rl.chain(rc.moved(rc.scene(3000, 3), 30.0, 40.0, 40.0), leaf, radius)) == 1
        if (leaf, radius) == (0.35, 0.1):
            assert (nn == 1).mean() > 0.8  # radius below the leaf: most centroids are alone
    assert seen == {1, 2, 3}


@pytest.fixture(scope="module")
def pack_results():
    pack = rc.ragged_pack()
    m, truth = rc.ragged_matches(pack)
    coarse, best, guesses = rc.synthetic_coarse(m, truth)
    whole = fl.fine(pack.clouds, m, None, fl.params(**fl.WHOLE), threads=THREADS)
    top = fl.fine(pack.clouds, m, guesses, fl.params(**fl.FINE), threads=THREADS)
    return pack, m, truth, (coarse, best, guesses), whole, top


def test_ragged_pack_reaches_the_groups_launches_and_edges(pack_results):
    pack, m, truth, (coarse, best, guesses), whole, top = pack_results
    lens = np.array([len(c) for c in pack.clouds])
    assert len(pack.clouds) == 600 and lens.max() == rc.MAX_LENGTH and (lens == rc.MAX_LENGTH).sum() >= 1
    assert rc.MAX_LENGTH & (rc.MAX_LENGTH - 1) == 0  # Kn == Pn == np2
    assert set(rc.FIXED_LENGTHS) <= set(lens.tolist())
    for i in range(pack.half):  # the second half: moved copies
        assert len(pack.clouds[pack.half + i]) == len(pack.clouds[i])
    sp = pack.special
    assert rc.finite_records(pack.clouds[sp["all_nan"]]) == 0 and len(pack.clouds[sp["all_nan"]]) > 0
    pn = pack.clouds[sp["part_nan"]]
    assert rc.finite_records(pn) == len(pn) - len(pn) // 10
    assert len(fl.voxel_irct(pack.clouds[sp["identical"]])) == 1
    ov = pack.clouds[sp["overflow"]]
    assert _same(fl.voxel_irct(ov), ov)  # leaf 0.2 is "too small": the output is the input
    assert (pack.clouds[sp["ground_only"]]["label"] == 0).all() and len(rl.chain(pack.clouds[sp["ground_only"]])) == 0
    assert {int(l) for c in pack.clouds[:20] for l in np.unique(c["label"])} == {-2, -1, 0, 1, 2}

    q, t = m["query_idx"].tolist(), m["match_idx"].tolist()
    pos = rc.slot_positions(m)
    assert len(m) > 2 * rc.PROBLEMS_PER_LAUNCH + 300
    assert len(pos) > 2 * rc.FINE_VOXEL_GROUP + 1
    assert set(pos) < set(range(len(pack.clouds)))  # some frame is named by no match
    for s in sp.values():
        assert s in q and s in t
    assert any(a == b for a, b in zip(q, t))
    recs = [r.tobytes() for r in m]
    assert len(set(recs)) < len(recs)  # exact duplicates
    assert set(q) - set(t) and set(t) - set(q)  # frames that are only ever source, only ever target
    # every voxel group and every launch holds problems with a known motion (a frame against its moved copy)
    known = [k for k in range(len(m)) if truth[k] is not None and q[k] != t[k]]
    assert {k // rc.PROBLEMS_PER_LAUNCH for k in known} == {0, 1, 2}
    assert {pos[q[k]] // rc.FINE_VOXEL_GROUP for k in known} == {0, 1, 2}

    bad_guess = [k for k in range(len(m)) if not np.isfinite(guesses[k]).all()
                 or abs(np.linalg.det(guesses[k][:3, :3].astype(np.float64)) - 1) > 0.1]
    assert len(bad_guess) >= 6 and max(bad_guess) >= rc.PROBLEMS_PER_LAUNCH
    assert set(np.unique(best).tolist()) == {0, 1}
    for name, res in (("whole", whole), ("top-part", top)):
        seen = set()
        for k in np.nonzero(res["state"] != bev_amd.ICP_NO_CORRESPONDENCES)[0]:
            seen |= {q[k], t[k]}
        missed = [f for f in pos if f not in seen and f not in pack.degenerate]
        assert not missed, f"{name}: frames in no compared registration: {missed}"
        states = set(np.unique(res["state"]).tolist())
        assert len(states) >= 3 and bev_amd.ICP_NO_CORRESPONDENCES in states, (name, states)
        assert states & {bev_amd.ICP_TRANSFORM, bev_amd.ICP_ABS_MSE, bev_amd.ICP_REL_MSE}, (name, states)
        assert res["iterations"].max() >= 5  # structure: several iterations
        # the known motions are found: the inputs are registrations, not noise
        err = [np.abs(res[k]["T"].reshape(4, 4)[:2, 3] - truth[k][:2, 3]).max() for k in known
               if min(len(pack.clouds[q[k]]), len(pack.clouds[t[k]])) >= 300 and q[k] not in sp.values()
               and q[k] - pack.half not in sp.values()]
        assert len(err) > 250 and np.median(err) < 0.05, (name, np.median(err))


def test_coarse_and_front_end_cases_reach_their_branches():
    pack = rc.ragged_pack()
    cf = rc.coarse_frames(pack, rl.chain)
    m = cf.matches
    named = set(m["query_idx"].tolist()) | set(m["match_idx"].tolist())
    assert 2 * len(m) > 2 * rc.PROBLEMS_PER_LAUNCH  # two problems per match: a third launch
    assert len(m) >= 1100
    assert cf.stride < cf.counts.max() and any(cf.counts[f] > cf.stride for f in named)
    assert any(cf.counts[f] > cf.stride for f in m["match_idx"].tolist())
    assert (m["query_idx"] == m["match_idx"]).any()
    empty = {f for f in range(len(cf.frames)) if cf.counts[f] == 0}
    assert empty & set(m["query_idx"].tolist()) and empty & set(m["match_idx"].tolist())
    assert [int(cf.counts[cf.hand[k]]) for k in ("rows0", "rows1", "rows2")] == [0, 1, 2]
    assert np.isnan(cf.frames[cf.hand["nan_normals"]][:, 4:7]).any()
    assert not np.isfinite(cf.frames[cf.hand["bad_points"]][:, :3]).all()

    fp = rc.front_pack(pack)
    by = dict(zip(fp.names, fp.clouds))
    big = rc.cell_counts(by["two_big_cells"])
    assert (big > rc.RF_LDS_KEYS).sum() == 2
    cnt = rc.cell_counts(by["cells_8192_8193_19_20"])
    assert sorted(cnt[cnt > 0].tolist()) == [rc.RF_MIN_CELL - 1, rc.RF_MIN_CELL, rc.RF_LDS_KEYS, rc.RF_LDS_KEYS + 1]
    worst = rc.cell_counts(by["cells_5k_plus_3"])
    assert (worst >= rc.RF_MIN_CELL).all() and (worst % 5 == 3).all()
    assert len(rl.top_part(by["cells_5k_plus_3"])) == int((worst // 5 + 1).sum())  # every cell rounds up
    for c in fp.clouds:
        assert len(rl.top_part(c)) <= len(c) // 5 + 51  # bev_regfront_max_out
    small = rc.small_frames()
    assert len(small) > 1024 and sum(len(rl.chain(c)) > 0 for c in small[:200]) > 20
