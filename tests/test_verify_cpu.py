"""The sequential checker of the verification calls (tests/verify/verify_oracle.c) against a numpy float64 brute
force that shares nothing with it, hand cases at the counting rule's boundary and over the empty and non-finite cases, and the
ground-truth world of ground_truth_cases.py, whose figures the DESIGN section quotes."""
import numpy as np
import pytest

import ground_truth_cases as gt
import verify_lib as vl
from bev_amd import VERIFY_RESULT_DTYPE, verify_params

F32, F64 = np.float32, np.float64
NAN, INF = F32(np.nan), F32(np.inf)


def brute64(src, tgt, T, thresholds):
    """(record, every finite nearest distance in metres) in float64: rows of (n, 3)"""
    T = np.asarray(T, F64).reshape(4, 4)
    q = np.asarray(src, F64).reshape(-1, 3) @ T[:3, :3].T + T[:3, 3]
    p = np.asarray(tgt, F64).reshape(-1, 3)
    qok, pok = np.isfinite(q).all(1), np.isfinite(p).all(1)
    rec = np.zeros(1, VERIFY_RESULT_DTYPE)[0]
    rec["n_query"], rec["n_target"] = qok.sum(), pok.sum()
    dists = []
    for a, aok, b, bok, name in ((q, qok, p, pok, "query_within"), (p, pok, q, qok, "target_within")):
        a, b = a[aok], b[bok]
        if not len(a) or not len(b):
            continue
        d2 = np.min(((a[:, None, :] - b[None, :, :]) ** 2).sum(2), axis=1)
        dists.append(np.sqrt(d2))
        for k, t in enumerate(thresholds):
            rec[name][k] = (d2 <= float(F32(t)) ** 2).sum()
    return rec, np.concatenate(dists) if dists else np.zeros(0)


LATTICE = [(1, 1), (7, 300), (300, 7), (257, 256), (600, 450)]
SHIFTS = [(0.0, 0.0, 0.0), (0.25, 0.0, 0.0), (-0.5, 0.125, 0.03125), (3.0, -2.0, 0.5)]
# Squared distances on the lattice are multiples of 1 / 1024, but never (7, 60 or 240) / 1024: no sum of three squares is
# 4^a (8 b + 7).  Thresholds at the roots of those leave 1 / 1024 to either side in d^2, more than 1e-3 in d up to 0.484 m; the
# last one is beyond every distance of the clouds.
THRESHOLDS = (float(np.sqrt(7 / 1024)), float(np.sqrt(60 / 1024)), float(np.sqrt(240 / 1024)), 100.0)


@pytest.mark.parametrize("ns,nt", LATTICE)
@pytest.mark.parametrize("shift", SHIFTS)
def test_oracle_equals_float64_brute_force(ns, nt, shift):
    tgt = vl.lattice(nt, 100 + nt, extent=8 * 32)
    # half of the source is the target's own points, so that the shifts land points exactly on points
    own = tgt[: min(ns // 2, nt)]
    src = np.concatenate([own, vl.lattice(ns - len(own), 200 + ns, extent=8 * 32)]).astype(F32)
    T = vl.shift4(*shift)
    want, d = brute64(src, tgt, T, THRESHOLDS)
    # the condition of the inputs: no distance within 1e-3 of a threshold, so float32 and float64 agree on every count
    assert all(np.abs(d - t).min() > 1e-3 for t in THRESHOLDS)
    got = vl.oracle(src, tgt, T, verify_params(THRESHOLDS))
    assert got.tobytes() == want.tobytes()


def test_identical_clouds_under_the_identity():
    c = vl.lattice(500, 1)
    r = vl.oracle(c, c, np.eye(4), verify_params((0.1, 0.2)))
    assert r["n_query"] == r["n_target"] == 500
    assert r["query_within"].tolist() == [500, 500, 0, 0, 0, 0, 0, 0] == r["target_within"].tolist()


def test_boundary_is_counted_at_equality_and_not_below():
    c = vl.lattice(200, 2, extent=400 * 32)  # sparse: no second point within 0.25 of a moved one
    T = vl.shift4(0.25)
    at = vl.oracle(c, c, T, verify_params((0.25,)))
    below = vl.oracle(c, c, T, verify_params((float(np.nextafter(F32(0.25), F32(0))),)))
    _, d = brute64(c, c, T, (0.25,))
    assert np.all(d == 0.25)
    assert at["query_within"][0] == at["target_within"][0] == 200
    assert below["query_within"][0] == below["target_within"][0] == 0


@pytest.mark.parametrize("bad", [NAN, INF])
def test_non_finite_transform(bad):
    c = vl.lattice(50, 3)
    T = np.eye(4, dtype=F32)
    T[1, 3] = bad
    r = vl.oracle(c, c, T, verify_params((0.1, 1.0)))
    assert r["n_query"] == 0 and r["n_target"] == 50
    assert not r["query_within"].any() and not r["target_within"].any()


def test_non_finite_points_and_negative_zero():
    c = vl.lattice(64, 4, extent=400 * 32)
    src, tgt = c.copy(), c.copy()
    src[0, 0], src[1, 1], src[2, 2] = NAN, INF, -INF
    src[3] = np.where(src[3] == 0, F32(-0.0), src[3])
    tgt[10, 2], tgt[11, 0] = NAN, -INF
    tgt[12] = [F32(-0.0), F32(-0.0), F32(0.0)]
    src[12] = [F32(0.0), F32(0.0), F32(-0.0)]
    r = vl.oracle(src, tgt, np.eye(4), verify_params((0.01,)))
    want, _ = brute64(src, tgt, np.eye(4), (0.01,))
    assert r.tobytes() == want.tobytes()
    assert r["n_query"] == 61 and r["n_target"] == 62
    assert r["query_within"][0] == 59 and r["target_within"][0] == 59  # 64 less the five points either side lost


def test_empty_sides():
    c = vl.lattice(20, 5)
    e = np.zeros((0, 3), F32)
    for src, tgt, nq, nt in ((e, c, 0, 20), (c, e, 20, 0), (e, e, 0, 0)):
        r = vl.oracle(src, tgt, np.eye(4), verify_params((1.0, 2.0)))
        assert (r["n_query"], r["n_target"]) == (nq, nt)
        assert not r["query_within"].any() and not r["target_within"].any()


def test_duplicates_count_once_each():
    c = vl.lattice(30, 6, extent=400 * 32)
    src = np.concatenate([c, c[:10]])
    r = vl.oracle(src, c, np.eye(4), verify_params((0.05,)))
    assert r["n_query"] == 40 and r["query_within"][0] == 40 and r["target_within"][0] == 30


@pytest.mark.parametrize("nt", [1, 8])
def test_threshold_counts_are_monotone_and_unused_slots_zero(nt):
    src, tgt = vl.lattice(300, 7), vl.lattice(280, 8)
    th = tuple(0.2 * 1.9 ** k for k in range(nt))
    r = vl.oracle(src, tgt, vl.shift4(0.125, -0.0625), verify_params(th))
    want, _ = brute64(src, tgt, vl.shift4(0.125, -0.0625), th)
    assert r.tobytes() == want.tobytes()
    for name in ("query_within", "target_within"):
        assert np.all(np.diff(r[name][:nt].astype(np.int64)) >= 0)
        assert not r[name][nt:].any()
    if nt == 8:
        assert r["query_within"][7] == 300 and r["target_within"][7] == 280


# ---- the ground-truth world: the figures of §6aa ---------------------------------------------------------
WORLD_T = (0.05, 0.1, 0.2, 0.3)


@pytest.fixture(scope="module")
def world():
    S = gt.setup()
    return S, {g: gt.ref_target(S, g)[1].astype(F32) for g in range(len(S["maps"]))}


@pytest.mark.parametrize("k", range(6))
def test_world_truth_counts_every_query_point_and_nothing_else(world, k):
    S, tgt = world
    q, g, _ = S["matches"][k]
    r = vl.oracle(S["xyz32"][q], tgt[g], S["truth"][k].astype(F32), verify_params(WORLD_T))
    assert r["n_query"] == len(S["xyz32"][q]) and r["n_target"] == len(tgt[g])
    assert r["query_within"][:4].tolist() == [r["n_query"]] * 4
    assert r["target_within"][:4].tolist() == [r["n_query"]] * 4


@pytest.mark.parametrize("k", range(6))
def test_world_far_off_explains_next_to_nothing(world, k):
    S, tgt = world
    q, g, _ = S["matches"][k]
    r = vl.oracle(S["xyz32"][q], tgt[g], gt.far_off(S, k), verify_params(WORLD_T))
    share = r["query_within"][3] / r["n_query"]
    print(f"match {k}: forward share at 0.3 m under far_off: {share:.4f}")
    assert share < 0.05  # measured: at most 0.022
