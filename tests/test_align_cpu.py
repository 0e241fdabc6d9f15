"""CPU: the sequential checker of the translation guess of retrieved pairs (tests/align/align_oracle.c) against
a numpy restatement of the contract that shares nothing with it — grids, every shift's score, the three orders, the offsets —
and on hand-made cases whose answers are known."""
import numpy as np
import pytest

import align_cases as ac
import align_lib
from bev_amd import POINT_DTYPE, align_params

F32 = np.float32
SHAPES = [(16, 2.0, 1, 0), (64, 0.5, 8, 1), (128, 0.5, 16, 3)]


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def np_grid(cloud, T, G, cell, skip, l2g=ac.L2G):
    """the height grid of a cloud under rows 0 ... 2 of T (None: the raw coordinates), array operations in float32"""
    x, y, z = (cloud[k].astype(F32) for k in "xyz")
    if T is not None:
        m = np.asarray(T, F32).reshape(-1)
        with np.errstate(all="ignore"):
            x, y, z = (m[4 * r] * x + (m[4 * r + 1] * y + (m[4 * r + 2] * z + m[4 * r + 3])) for r in range(3))
    with np.errstate(all="ignore"):
        ok = (x * x + y * y) > 0
        fx, fy = np.floor(x / F32(cell)), np.floor(y / F32(cell))
        h = F32(G // 2)
        ok &= (-h <= fx) & (fx < h) & (-h <= fy) & (fy < h)
        if skip:
            ok &= cloud["label"] != 0
        u = (z + F32(l2g)) * F32(4.0)
        v = np.where((u >= F32(-2147483648.0)) & (u < F32(2147483648.0)), np.trunc(np.where(np.isfinite(u), u, 0)), -1.0)
    v = np.clip(v, 0, 127).astype(np.uint8)
    g = np.zeros((G, G), np.uint8)
    ix, iy = fx[ok].astype(np.int64) + G // 2, fy[ok].astype(np.int64) + G // 2
    np.maximum.at(g, (iy, ix), v[ok])
    return g


def np_scores(q, c, S):
    G = q.shape[0]
    pad = np.zeros((G + 2 * S, G + 2 * S), np.int64)
    pad[S: S + G, S: S + G] = c
    q = q.astype(np.int64)
    return np.array([[(q * pad[S + dy: S + dy + G, S + dx: S + dx + G]).sum() for dx in range(-S, S + 1)]
                     for dy in range(-S, S + 1)], np.int64)


def np_best_shift(sc, S):
    keys = [(-int(sc[dy + S, dx + S]), dx * dx + dy * dy, dy, dx) for dy in range(-S, S + 1) for dx in range(-S, S + 1)]
    _, _, dy, dx = min(keys)
    return dx, dy


def np_offset(d, S, sm, s0, sp):
    if d - 1 < -S or d + 1 > S:
        return 0.0
    den = float(sm) - 2.0 * float(s0) + float(sp)
    off = 0.5 * (float(sm) - float(sp)) / den if den < 0 else 0.0
    return min(0.5, max(-0.5, off))


def np_hit(query, cgrid, angle, prm):
    """(results' T[3], T[7], fitness, converged per flip; best; detail tuples) from the restatement; the rotation is the
    checker's align_guess (bev_libm_f64.h has its own tests)"""
    G, S, K = prm.grid, prm.max_shift, prm.yaw_steps
    c = np.zeros((G, G), np.uint8) if cgrid is None else cgrid
    out, top = [], []
    for flip in (0, 1):
        cands = []
        for k in range(-K, K + 1):
            T = align_lib.guess(angle, k, prm.yaw_step, flip)
            q = np_grid(query, T, G, prm.cell, prm.skip_label0)
            sc = np_scores(q, c, S)
            dx, dy = np_best_shift(sc, S)
            cands.append((-int(sc[dy + S, dx + S]), abs(k), k, dx, dy, sc, q, T))
        s, _, k, dx, dy, sc, q, T = min(cands, key=lambda t: t[:3])
        s = -s
        at = lambda x, y: sc[y + S, x + S] if abs(x) <= S and abs(y) <= S else 0
        ox = np_offset(dx, S, at(dx - 1, dy), s, at(dx + 1, dy))
        oy = np_offset(dy, S, at(dx, dy - 1), s, at(dx, dy + 1))
        eq, ec = int((q.astype(np.int64) ** 2).sum()), int((c.astype(np.int64) ** 2).sum())
        fit = 1.0 - s / np.sqrt(float(eq) * float(ec)) if s > 0 else 2.0
        out.append(dict(T=T, tx=F32((dx + ox) * float(F32(prm.cell))), ty=F32((dy + oy) * float(F32(prm.cell))), fitness=fit,
                        converged=int(s > 0), dx=dx, dy=dy, k=k, score=s, eq=eq, ec=ec, off_x=F32(ox), off_y=F32(oy)))
        top.append(s)
    return out, 0 if top[0] >= top[1] else 1


def check_hit(query, cgrid, angle, prm):
    res, best, det = align_lib.hit(query, cgrid, angle, prm)
    want, want_best = np_hit(query, cgrid, F32(angle), prm)
    assert best == want_best
    for flip in (0, 1):
        w, r, d = want[flip], res[flip], det[flip]
        T = w["T"].copy()
        T[3], T[7] = w["tx"], w["ty"]
        assert r["T"].tobytes() == T.tobytes(), (flip, r["T"], T)
        assert r["fitness"] == w["fitness"] and r["converged"] == w["converged"]
        assert (r["iterations"], r["state"], r["_pad"]) == (0, 0, 0)
        assert (d["dx"], d["dy"], d["k"], d["flip"], d["score"], d["eq"], d["ec"]) == \
               (w["dx"], w["dy"], w["k"], flip, w["score"], w["eq"], w["ec"])
        assert d["off_x"] == w["off_x"] and d["off_y"] == w["off_y"]
    return res, best, det


# ---- the checker against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skip", [True, False])
@pytest.mark.parametrize("G,cell,S,K", SHAPES)
def test_grids(G, cell, S, K, skip):
    prm = align_params(G, cell, S, K, 2.0, skip)
    rng = np.random.default_rng([31, G])
    frames = [ac.seeded(rng, n, G, cell) for n in (0, 1, 257, 3000)] + [ac.edge_frame(G, cell)]
    mats = [None, ac.rigid12(1.5, -2.0, 33.0, [0.3 * G * cell, -0.1 * G * cell, 0.4]), ac.rigid12(0, 0, 180.0, [0, 0, 0])]
    for f in frames:
        for m in mats:
            assert np.array_equal(align_lib.grid([(f, m)], prm), np_grid(f, m, G, cell, skip))
    both = align_lib.grid([(frames[3], mats[1]), (frames[2], None)], prm)
    assert np.array_equal(both, np.maximum(np_grid(frames[3], mats[1], G, cell, skip), np_grid(frames[2], None, G, cell, skip)))
    assert align_lib.energy(both) == int((both.astype(np.int64) ** 2).sum())
    if skip:
        assert not np.array_equal(align_lib.grid([(frames[3], None)], prm),
                                  align_lib.grid([(frames[3], None)], align_params(G, cell, S, K, 2.0, False)))


def test_edge_points_fall_where_the_float_comparison_says():
    G, cell = 16, 2.0
    prm = align_params(G, cell, 1, 0, 0.0, False)
    up, down = F32(np.inf), F32(-np.inf)
    lo, hi = F32(-16.0), F32(16.0)
    for x, col in ((lo, 0), (np.nextafter(lo, down), None), (np.nextafter(lo, up), 0), (hi, None), (np.nextafter(hi, down), 15),
                   (F32(2.0), 9), (np.nextafter(F32(2.0), down), 8), (np.nextafter(F32(2.0), up), 9), (F32(-0.0), 8),
                   (F32(np.nan), None), (F32(np.inf), None), (F32(-np.inf), None), (F32(-1e-30), 7)):
        g = align_lib.grid([(ac.cloud_of([(x, 1.0)]), None)], prm)
        assert np.array_equal(g, np_grid(ac.cloud_of([(x, 1.0)]), None, G, cell, 0))
        if col is None:
            assert not g.any(), x
        else:
            assert g[8, col] == 12 and np.count_nonzero(g) == 1, (x, col)   # (1.0 + 2.0) * 4
        gy = align_lib.grid([(ac.cloud_of([(1.0, x)]), None)], prm)
        assert np.array_equal(gy, g.T)
    assert not align_lib.grid([(ac.cloud_of([(0.0, 0.0), (-0.0, 0.0)]), None)], prm).any()  # the origin's no-return records


@pytest.mark.parametrize("G,cell,S,K", SHAPES)
def test_scores_of_every_shift(G, cell, S, K):
    prm = align_params(G, cell, S, K, 2.0, True)
    rng = np.random.default_rng([32, G])
    q = align_lib.grid([(ac.seeded(rng, 2000, G, cell), None)], prm)
    c = align_lib.grid([(ac.seeded(rng, 2500, G, cell), None)], prm)
    full = rng.integers(100, 128, (G, G)).astype(np.uint8)
    for a, b in ((q, c), (full, full), (q, np.zeros_like(q)), (np.zeros_like(q), c)):
        sc = align_lib.scores(a, b, S)
        assert np.array_equal(sc.astype(np.int64), np_scores(a, b, S))
    assert int(align_lib.scores(np.full((128, 128), 127, np.uint8), np.full((128, 128), 127, np.uint8), 16)[16, 16]) == 128 * 128 * 127 * 127


@pytest.mark.parametrize("G,cell,S,K,step", [(16, 2.0, 1, 0, 0.0), (64, 0.5, 8, 1, 2.0), (32, 1.0, 4, 3, 0.0), (32, 1.0, 4, 2, 1.5)])
def test_hits_against_the_restatement(G, cell, S, K, step):
    prm = align_params(G, cell, S, K, step, True)
    rng = np.random.default_rng([33, G, K])
    cand = ac.seeded(rng, 3000, G, cell)
    cgrid = align_lib.grid([(cand, None)], prm)
    for yaw, tx, ty, angle in ((0.0, 0.0, 0.0, 0.0), (30.0, 1.7 * cell, -0.6 * cell, 31.0), (-120.0, -0.4 * S * cell, 0.3 * S * cell, 58.5),
                               (179.0, 0.2, 0.1, -1.5)):
        check_hit(ac.moved(cand, yaw, tx, ty), cgrid, angle, prm)
    check_hit(ac.seeded(rng, 500, G, cell), cgrid, 77.0, prm)
    for bad in (np.nan, np.inf, 3e9):  # no rotation: T is NaN, nothing contributes
        res, best, det = check_hit(cand, cgrid, bad, prm)
        assert best == 0 and det["score"].tolist() == [0, 0] and res["fitness"].tolist() == [2.0, 2.0]


# ---- hand-made cases -----------------------------------------------------------------------------------------------------------------
def _blob(G, cell, rng, n=40, spread=0.2):
    """points in distinct cells within spread * G cells of the centre, at cell centres (no point near an edge), distinct heights"""
    r = int(spread * G)
    n = min(n, (2 * r) ** 2 // 2)
    cells = rng.permutation((2 * r) ** 2)[:n]
    ix, iy = cells % (2 * r) - r, cells // (2 * r) - r
    c = ac.cloud_of(np.c_[(ix + 0.5) * cell, (iy + 0.5) * cell], z=rng.uniform(0.0, 20.0, n).astype(F32))
    return c


@pytest.mark.parametrize("G,cell,S", [(16, 2.0, 1), (64, 0.5, 8), (128, 0.5, 16)])
def test_a_grid_against_itself_moved_by_whole_cells(G, cell, S):
    """the query is the candidate moved by (mx, my) whole cells: the shift comes back, with offset 0, at exactly +-S as well
    (no neighbour beyond the window) and inside it (the autocorrelation is symmetric)"""
    prm = align_params(G, cell, S, 0, 0.0, True)
    rng = np.random.default_rng([34, G])
    cand = _blob(G, cell, rng)
    cgrid = align_lib.grid([(cand, None)], prm)
    moves = [(S, 0), (-S, 0), (0, S), (0, -S), (S, -S), (1, 0), (0, -1), (0, 0)] + ([(3, -2), (-S + 1, S - 1)] if S > 3 else [])
    for mx, my in moves:
        q = cand.copy()
        q["x"] -= F32(mx * cell)
        q["y"] -= F32(my * cell)
        res, best, det = check_hit(q, cgrid, 0.0, prm)
        d = det[0]
        assert (d["dx"], d["dy"], d["off_x"], d["off_y"]) == (mx, my, 0.0, 0.0), (mx, my, d)
        assert d["score"] == d["eq"] == d["ec"] and best == 0 and res[0]["fitness"] == 0.0 and res[0]["converged"] == 1
        assert res[0]["T"][3] == F32(mx * cell) and res[0]["T"][7] == F32(my * cell)
        assert res[0]["T"].tolist()[:3] == [1.0, 0.0, 0.0] and res[0]["T"][15] == 1.0


def test_equal_scores_go_to_the_nearer_shift_and_then_to_the_order():
    G, cell, S = 32, 1.0, 4
    prm = align_params(G, cell, S, 0, 0.0, True)
    q = ac.cloud_of([(0.5, 0.5)], z=3.0)
    for pts, want in (([(2.5, 0.5), (-0.5, 0.5)], (-1, 0)),        # 2 to the right, 1 to the left: the nearer
                      ([(2.5, 0.5), (-1.5, 0.5)], (-2, 0)),        # the same distance: the smaller dx
                      ([(0.5, 2.5), (2.5, 0.5)], (0, 2)[::-1]),    # the same distance on two axes: the smaller dy wins -> (2, 0)
                      ([(0.5, -1.5), (-1.5, 0.5), (2.5, 0.5), (0.5, 2.5)], (0, -2))):
        cgrid = align_lib.grid([(ac.cloud_of(pts, z=3.0), None)], prm)
        _, _, det = check_hit(q, cgrid, 0.0, prm)
        assert (det[0]["dx"], det[0]["dy"]) == want, (pts, det[0])
    # among the k of a flip: yaw_step 0 makes every k the same hypothesis, k = 0 wins
    prm = align_params(G, cell, S, 3, 0.0, True)
    _, _, det = check_hit(q, align_lib.grid([(q, None)], prm), 0.0, prm)
    assert det["k"].tolist() == [0, 0]


def test_empty_query_empty_candidate_and_no_candidate():
    G, cell, S = 32, 1.0, 4
    prm = align_params(G, cell, S, 1, 2.0, True)
    rng = np.random.default_rng(35)
    cand = ac.seeded(rng, 800, G, cell)
    cgrid = align_lib.grid([(cand, None)], prm)
    empty = np.zeros(0, POINT_DTYPE)
    for query, cg in ((empty, cgrid), (cand, np.zeros_like(cgrid)), (cand, None), (empty, None)):
        res, best, det = check_hit(query, cg, 12.0, prm)
        assert best == 0
        for flip in (0, 1):
            assert (det[flip]["dx"], det[flip]["dy"], det[flip]["k"], det[flip]["score"]) == (0, 0, 0, 0)
            assert res[flip]["fitness"] == 2.0 and res[flip]["converged"] == 0 and res[flip]["T"][3] == 0.0 and res[flip]["T"][7] == 0.0
            assert np.array_equal(res[flip]["T"], align_lib.guess(12.0, 0, 2.0, flip))
    assert det[0]["eq"] == 0 and align_lib.hit(cand, None, 12.0, prm)[2][0]["eq"] > 0 and align_lib.hit(cand, None, 12.0, prm)[2][0]["ec"] == 0


def test_a_single_point_and_the_flip():
    G, cell, S = 32, 1.0, 4
    prm = align_params(G, cell, S, 0, 0.0, True)
    cgrid = align_lib.grid([(ac.cloud_of([(3.5, -2.5)], z=5.0), None)], prm)
    res, best, det = check_hit(ac.cloud_of([(2.5, -0.5)], z=1.0), cgrid, 0.0, prm)
    assert best == 0 and (det[0]["dx"], det[0]["dy"]) == (1, -2) and det[0]["score"] == 28 * 12
    assert det[1]["score"] == 0          # turned by half a circle the point lies at (-2.5, 0.5): 6 cells from the candidate
    res, best, det = check_hit(ac.cloud_of([(-2.5, 0.5)], z=1.0), cgrid, 0.0, prm)
    assert best == 1 and det[1]["score"] == 28 * 12
    # label 0 on and off
    q0 = ac.cloud_of([(2.5, -0.5)], z=1.0, label=0)
    assert align_lib.hit(q0, cgrid, 0.0, prm)[2][0]["score"] == 0
    assert align_lib.hit(q0, cgrid, 0.0, align_params(G, cell, S, 0, 0.0, False))[2][0]["score"] == 28 * 12


def test_the_offset_follows_the_parabola():
    G, cell, S = 32, 1.0, 4
    prm = align_params(G, cell, S, 0, 0.0, True)
    # the candidate's one column of heights 10, 20, 12 (codes 48, 88, 56) against one query cell: S- = 48 v, S0 = 88 v, S+ = 56 v
    cgrid = align_lib.grid([(ac.cloud_of([(0.5, 0.5), (1.5, 0.5), (2.5, 0.5)], z=np.array([10.0, 20.0, 12.0], F32)), None)], prm)
    _, _, det = check_hit(ac.cloud_of([(0.5, 0.5)], z=1.0), cgrid, 0.0, prm)
    assert (det[0]["dx"], det[0]["dy"]) == (1, 0)
    assert det[0]["off_x"] == F32(0.5 * (48 - 56) / (48 - 176 + 56)) and det[0]["off_y"] == 0.0


def test_parameters():
    assert align_lib.admitted(align_params())
    for bad in (align_params(grid=14), align_params(grid=130), align_params(grid=65), align_params(cell=0.0), align_params(cell=-1.0),
                align_params(cell=float("nan")), align_params(cell=float("inf")), align_params(max_shift=0), align_params(max_shift=17),
                align_params(grid=32, max_shift=9), align_params(yaw_steps=-1), align_params(yaw_steps=4), align_params(yaw_step=-0.5),
                align_params(yaw_step=float("nan")), align_params(yaw_step=float("inf"))):
        assert not align_lib.admitted(bad)
    for ok in (align_params(16, 1.0, 4, 0, 0.0), align_params(32, 1.0, 8), align_params(128, 0.1, 16, 3, 0.0)):
        assert align_lib.admitted(ok)
