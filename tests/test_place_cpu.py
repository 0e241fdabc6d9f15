"""CPU: the sequential checker of place retrieval (tests/place/place_oracle.c) against a plain numpy
restatement of the contract, its edge properties, and the ground-truth case through the checker alone."""
import functools

import numpy as np
import pytest

import place_cases
import place_lib
from bev_amd import POINT_DTYPE, place_params

SHAPES = [(20, 60), (4, 8), (32, 64)]


def np_units(desc):
    """(unit (R, C) int64, nonempty (C,) bool): a column scaled to length 127, rounded half up, in float64"""
    v = desc.astype(np.int64)
    n2 = (v * v).sum(axis=0)
    unit = np.floor(127.0 * v / np.sqrt(np.maximum(n2, 1).astype(np.float64)) + 0.5).astype(np.int64)
    return np.where(n2 > 0, unit, 0), n2 > 0


def np_shifts(dq, dc):
    uq, eq = np_units(dq)
    uc, ec = np_units(dc)
    C = dq.shape[1]
    S = np.array([(uq * np.roll(uc, -n, axis=1)).sum() for n in range(C)])
    cnt = np.array([(eq & np.roll(ec, -n)).sum() for n in range(C)])
    return S, cnt


def better(a, b):
    """(S, cnt, index) records: the contract's comparison"""
    if (a[1] == 0) != (b[1] == 0):
        return a[1] > 0
    if a[1] and int(a[0]) * int(b[1]) != int(b[0]) * int(a[1]):
        return int(a[0]) * int(b[1]) > int(b[0]) * int(a[1])
    return a[2] < b[2]


def np_match(dq, ddb, top_k, limit=None):
    C = dq.shape[2]
    out = []
    for q in range(len(dq)):
        recs = []
        for c in range(len(ddb) if limit is None else limit[q]):
            S, cnt = np_shifts(dq[q], ddb[c])
            best = 0
            for n in range(1, C):
                if better((S[n], cnt[n], n), (S[best], cnt[best], best)):
                    best = n
            recs.append((S[best], cnt[best], c, best))
        recs.sort(key=functools.cmp_to_key(lambda a, b: -1 if better(a, b) else 1))
        row = []
        for k in range(top_k):
            if k < len(recs):
                S, cnt, c, n = recs[k]
                ang = n * (360.0 / C)
                row.append((q, c, ang - 360.0 if ang >= 180.0 else ang, n, 1.0 - S / (16129.0 * cnt) if cnt else 2.0))
            else:
                row.append((q, -1, 0.0, 0, 2.0))
        out.append(row)
    return out


def seeded(rng, R, C, n, density):
    d = rng.integers(0, 128, (n, R, C)).astype(np.uint8)
    d[rng.uniform(size=(n, R, C)) >= density] = 0
    d[:, :, rng.uniform(size=C) < 0.2] = 0  # empty columns, the same in all
    return d


@pytest.mark.parametrize("R,C", SHAPES)
def test_checker_equals_numpy(R, C):
    rng = np.random.default_rng([7, R, C])
    dq, ddb = seeded(rng, R, C, 5, 0.5), seeded(rng, R, C, 9, 0.3)
    ddb[3] = ddb[1]
    ddb[6] = 0
    for q in range(2):
        for c in (0, 3, 6):
            S, cnt = place_lib.pair_shifts(dq[q], ddb[c])
            S_np, cnt_np = np_shifts(dq[q], ddb[c])
            assert np.array_equal(S, S_np) and np.array_equal(cnt, cnt_np)
    limit = np.array([9, 0, 1, 4, 9], np.int32)
    for top_k, lim in ((1, None), (3, limit), (12, limit)):
        hits = place_lib.match(dq, ddb, top_k, lim)
        want = np_match(dq, ddb, top_k, lim)
        for q in range(len(dq)):
            for k in range(top_k):
                h, w = hits[q, k], want[q][k]
                assert (h["query_idx"], h["match_idx"], h["shift"]) == w[:2] + w[3:4]
                assert h["angle_guess"] == np.float32(w[2]) and h["distance"] == w[4]


@pytest.mark.parametrize("R,C", SHAPES)
def test_rolled_copy_gives_the_shift(R, C):
    """One non-zero ring per column: every unit value is 127 exactly, so the rolled copy's distance is 0.0 exactly.  A dense
    descriptor's columns have sums of squares of 16129 +- (sum of |rounding| <= 0.5 per ring): |distance| <=
    (127 sqrt(R) + R / 4) / 16129."""
    rng = np.random.default_rng([8, R, C])
    one = np.zeros((R, C), np.uint8)
    one[rng.integers(0, R, C), np.arange(C)] = rng.integers(1, 128, C)
    dense = rng.integers(1, 128, (R, C)).astype(np.uint8)
    for n in (0, 1, C // 2 - 1, C // 2, C - 1):
        for d, bound in ((one, 0.0), (dense, (127.0 * np.sqrt(R) + R / 4) / 16129.0)):
            h = place_lib.match(d[None], np.roll(d, n, axis=1)[None])[0, 0]
            ang = n * 360.0 / C
            assert h["shift"] == n and h["match_idx"] == 0
            assert h["angle_guess"] == np.float32(ang - 360.0 if ang >= 180.0 else ang)
            assert abs(h["distance"]) <= bound


def test_ties_go_to_the_lower_index_and_zero_is_far():
    rng = np.random.default_rng(9)
    d = seeded(rng, 20, 60, 3, 0.5)
    db = np.stack([d[1], d[0], d[2], d[0], np.zeros_like(d[0])])
    hits = place_lib.match(d[:1], db, top_k=5)[0]
    assert list(hits["match_idx"][:2]) == [1, 3] and hits["distance"][0] == hits["distance"][1]
    assert hits["match_idx"][4] == 4 and hits["distance"][4] == 2.0 and hits["shift"][4] == 0
    zero = place_lib.match(np.zeros((1, 20, 60), np.uint8), db, top_k=2)[0]
    assert list(zero["match_idx"]) == [0, 1] and list(zero["distance"]) == [2.0, 2.0]


def test_descriptor_of_hand_made_points():
    """ring edges, sector edges, the origin, NaN / inf, label 0, the height clamp: each point placed by hand"""
    p = place_params(4, 8, 8.0, True)  # rings of 2 m, sectors of 45 degrees
    pts = np.zeros(9, POINT_DTYPE)
    pts["label"] = 1
    pts["x"], pts["y"], pts["z"] = [1, 2, 0, -3, 0, 8, np.nan, 1, 5], [0, 0, 5, 0, 0, 0, 1, 1, -5], [0, 50, -0.5, -3, 9, 9, 9, np.inf, 1]
    pts["label"][8] = 0
    d = place_lib.descriptor([(pts, None)], p)
    want = np.zeros((4, 8), np.uint8)
    want[0, 0] = 8      # (1, 0, 0): ring 0, sector 0, (0 + 2) * 4
    want[1, 0] = 127    # (2, 0, 50): r2 == edge2[1] belongs to ring 1; the clamp
    want[2, 2] = 6      # (0, 5, -0.5): 90 degrees is sector 2's lower edge
    want[1, 4] = 0      # (-3, 0, -3): 180 degrees, sector 4; a negative height is 0
    assert np.array_equal(d, want)  # the origin, r2 == edge2[4], NaN, inf z (value 0) and label 0 leave nothing
    d0 = place_lib.descriptor([(pts, None)], place_params(4, 8, 8.0, False))
    assert d0[3, 7] == 12 and np.array_equal(np.delete(d0.ravel(), 31), np.delete(want.ravel(), 31))


def test_ground_truth_case_is_discriminative():
    """A condition on the inputs: through the checker alone every query's best candidate is its own frame, and the runner-up
    is at least 0.05 behind."""
    S = place_cases.case()
    p = place_cases.params()
    db = np.stack([place_lib.descriptor([(c, None)], p) for c in S["db_clouds"]])
    dq = np.stack([place_lib.descriptor([(c, None)], p) for c in S["q_clouds"]])
    hits = place_lib.match(dq, db, top_k=2)
    margin = hits["distance"][:, 1] - hits["distance"][:, 0]
    print("best distance <=", hits["distance"][:, 0].max(), "margin >=", margin.min())
    assert np.array_equal(hits["match_idx"][:, 0], S["truth"])
    assert margin.min() >= 0.05
    for h, t in zip(hits[:, 0], S["turn"]):
        assert place_cases.angle_error(h["angle_guess"], t) <= place_cases.SECTOR_DEG
