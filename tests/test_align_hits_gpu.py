"""GPU: the results, best and detail of bev_align_hits_device_resident and bev_align_batch, byte for byte
against the sequential checker (tests/align/align_oracle.c): hit lists of 1 to 130 hits over 5 queries and 7 candidates, among
them repeated hits, hits without a match, an empty query and queries made by moving a candidate by a known yaw and offset; one
call against two calls over halves and against launch groups of 7; the host-buffer form; every refusal."""
import functools
import os

import numpy as np
import pytest

import align_cases as ac
import align_lib
import bev_amd
from align_gpu_lib import checker_grids, guarded, hits
from bev_amd import MATCH_DTYPE, POINT_DTYPE, align_params
from packed_cases import _p

pytestmark = pytest.mark.gpu
SHAPES = [(16, 2.0, 1, 0), (64, 0.5, 8, 1), (128, 0.5, 16, 3)]
LENGTHS = (1, 2, 33, 130)
MOVES = {0: (0, 20.0, 1.3, -2.2), 1: (3, -100.0, -0.7, 0.4), 4: (5, 190.0, 0.45, 0.8)}  # query: (candidate, yaw, offset in cells)


@pytest.fixture(scope="module")
def ctx():
    c = bev_amd.BevContext(_p(), device=0, max_batch=4)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _case(G, cell, S):
    """(queries (5), candidates (7), hits (130,) MATCH_DTYPE): queries 0, 1 and 4 are candidates moved by a known yaw and offset
    (4 by more than half a circle: its true flip is 1), 2 is its own cloud, 3 is empty; a hit's angle depends on its pair alone,
    so equal pairs are repeated hits; every ninth hit found nothing"""
    rng = np.random.default_rng([51, G])
    cands = [ac.seeded(rng, n, G, cell) for n in (3000, 1, 257, 2000, 0, 4000, 1025)]
    queries = []
    for q in range(5):
        if q in MOVES:
            c, yaw, ox, oy = MOVES[q]
            queries.append(ac.moved(cands[c], yaw, min(ox, S - 0.5) * cell, max(oy, -S + 0.5) * cell))
        else:
            queries.append(ac.seeded(rng, 1500, G, cell) if q == 2 else np.zeros(0, POINT_DTYPE))
    base = {0: 20.0, 1: -99.0, 2: 63.0, 3: 5.0, 4: 11.0}
    pairs = [(0, 0), (4, 5), (1, 3)] + [(int(q), int(c)) for q, c in zip(rng.integers(0, 5, 127), rng.integers(0, 7, 127))]
    m = np.zeros(130, MATCH_DTYPE)
    for i, (q, c) in enumerate(pairs):
        m[i] = (q, -1 if i % 9 == 8 else c, np.float32(base[q] + 0.25 * c))
    m[10] = m[0]
    m[40]["match_idx"] = -7
    return queries, cands, m


@functools.lru_cache(maxsize=None)
def _want(G, cell, S, K, step):
    prm = align_params(G, cell, S, K, step, True)
    queries, cands, m = _case(G, cell, S)
    cgrids = checker_grids(cands, prm)
    return cgrids, align_lib.hits(queries, cgrids, m, prm)


def _same(got, want, n=None):
    for g, w in zip(got, want):
        assert g.tobytes() == (w if n is None else w[:n]).tobytes()


@pytest.mark.parametrize("step", [0.0, 2.0])
@pytest.mark.parametrize("G,cell,S,K", SHAPES)
def test_hit_lists_against_the_checker(ctx, G, cell, S, K, step):
    prm = align_params(G, cell, S, K, step, True)
    queries, cands, m = _case(G, cell, S)
    cgrids, want = _want(G, cell, S, K, step)
    res, best, det = want
    # the inputs do what they are meant to: the moved candidates come back where they were put, query 4 under flip 1
    # (the grid of 16 x 16 cells is full of the seeded points: its answers are checked against the checker alone)
    assert S < 8 or ((det[0, 0]["dx"], det[0, 0]["dy"]) == (1, -2) and best[0] == 0 and best[1] == 1)
    assert res[0, 0]["converged"] == 1
    assert det[8, 0]["score"] == 0 and det[8, 0]["ec"] == 0 and res[8, 0]["fitness"] == 2.0
    for n in LENGTHS:
        _same(hits(ctx, queries, cgrids, m[:n], prm), want, n)
    _same(hits(ctx, queries, cgrids, m, prm, pieces=2), want)
    only = hits(ctx, queries, cgrids, m[:33], prm, want_detail=False)
    assert only[2] is None
    _same(only[:2], want[:2], 33)
    os.environ["BEV_ALIGN_GROUP"] = "7"
    try:
        _same(hits(ctx, queries, cgrids, m, prm), want)
    finally:
        del os.environ["BEV_ALIGN_GROUP"]


@pytest.mark.parametrize("G,cell,S,K", SHAPES[:2])
def test_the_host_buffer_form(ctx, G, cell, S, K):
    """the frames are queries and candidates at once: the candidates' list, hits over it"""
    prm = align_params(G, cell, S, K, 2.0, True)
    _, cands, _ = _case(G, cell, S)
    frames = cands + [ac.moved(cands[0], 15.0, 0.9 * cell, -0.3 * cell)]
    m = np.array([(7, 0, 14.0), (0, 0, 0.0), (2, 5, 33.0), (4, 3, -8.0), (7, -1, 14.0), (3, 7, 1.0)], MATCH_DTYPE)
    cgrids = checker_grids(frames, prm)
    want = align_lib.hits(frames, cgrids, m, prm)
    _same(hits(ctx, frames, cgrids, m, prm), want)
    _same(ctx.align_batch(frames, m, prm), want)
    got = ctx.align_batch(frames, m, prm, want_detail=False)
    assert got[2] is None
    _same(got[:2], want[:2])
    # against maps: map 0 is frame 0 under the identity, map 1 frames 3 and 5 under rigid matrices
    offs, ef = np.array([0, 1, 3], np.uint64), np.array([0, 3, 5], np.int32)
    ep = np.stack([np.eye(3, 4, dtype=np.float32).reshape(12), ac.rigid12(0.5, -1.0, 40.0, [cell, 2 * cell, 0.1]),
                   ac.rigid12(0, 0, -75.0, [-3 * cell, 0, 0])])
    mm = np.array([(7, 0, 14.0), (3, 1, 2.0), (5, 1, -70.0), (1, -1, 0.0)], MATCH_DTYPE)
    mgrids = checker_grids(frames, prm, maps=(offs, ef, ep))
    assert mgrids[0].tobytes() == cgrids[0].tobytes()
    _same(ctx.align_batch(frames, mm, prm, map_offsets=offs, entry_frame=ef, entry_pose=ep), align_lib.hits(frames, mgrids, mm, prm))
    assert len(ctx.align_batch(frames, np.zeros(0, MATCH_DTYPE), prm)[0]) == 0


def test_refusals(ctx):
    G, cell, S = 16, 2.0, 1
    prm = align_params(G, cell, S, 0, 0.0, True)
    queries, cands, m = _case(G, cell, S)
    cgrids = checker_grids(cands, prm)
    for bad in (align_params(14), align_params(130), align_params(cell=0.0), align_params(max_shift=0), align_params(32, 1.0, 9),
                align_params(yaw_steps=-1), align_params(yaw_steps=4), align_params(yaw_step=float("nan")),
                bev_amd.AlignParams(16, 2.0, 1, 0, 0.0, 2)):
        with pytest.raises(bev_amd.BevError):
            hits(ctx, queries, cgrids, m[:3], bad)
        with pytest.raises(bev_amd.BevError):
            ctx.align_batch(queries, m[:3], bad)
    for q, c in ((5, 0), (-1, 0), (0, 7)):  # an index out of range
        with pytest.raises(bev_amd.BevError):
            hits(ctx, queries, cgrids, np.array([(0, 0, 0.0), (q, c, 0.0)], MATCH_DTYPE), prm)
    with pytest.raises(bev_amd.BevError):  # bev_align_batch: the candidates are the 5 frames
        ctx.align_batch(queries, np.array([(0, 5, 0.0)], MATCH_DTYPE), prm)
    d = guarded(4096)
    offs = np.array([0, 4, 8], np.uint64)
    one = np.array([(0, 0, 0.0)], MATCH_DTYPE)
    args = dict(n_frames=2, d_clouds=d.data_ptr(), offsets=offs, n_db=1, d_grids=d.data_ptr(), d_energy=d.data_ptr(), hits=one,
                d_results=d.data_ptr(), d_best=d.data_ptr(), d_detail=0, params=prm)
    for k, v in (("d_results", 0), ("d_best", 0), ("d_grids", 0), ("d_energy", 0), ("d_clouds", 0), ("n_db", -1),
                 ("offsets", np.array([0, 8, 4], np.uint64))):
        with pytest.raises(bev_amd.BevError):
            ctx.align_hits_device(**{**args, k: v})
    # a hit without a match needs no grids; no hits need nothing
    ctx.align_hits_device(**{**args, "hits": np.array([(1, -1, 0.0)], MATCH_DTYPE), "d_grids": 0, "d_energy": 0, "n_db": 0})
    ctx.align_hits_device(**{**args, "hits": np.zeros(0, MATCH_DTYPE), "d_results": 0, "d_best": 0})
    ctx.synchronize()
