"""GPU: the hits of bev_place_match_device_resident, byte for byte against the sequential checker
(tests/place/place_oracle.c): sizes past one tile of candidates and one group of queries, every top_k, limits, sparse, dense,
duplicate, rolled and all-zero descriptors, and the same hits whatever the split of the queries."""
import functools
import os

import numpy as np
import pytest

import bev_amd
import place_lib
from bev_amd import PLACE_HIT_DTYPE, place_params
from packed_cases import _p
from place_gpu_lib import handles, match

pytestmark = pytest.mark.gpu
SIZES = (1, 2, 33, 65, 130)


@pytest.fixture(scope="module")
def ctx():
    c = bev_amd.BevContext(_p(), device=0, max_batch=2)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _pool(R, C):
    """130 query and 130 database descriptors: sparse ones with empty columns, dense ones, duplicates, rolled copies of
    queries, an all-zero one on either side; with their records"""
    rng = np.random.default_rng([12, R, C])
    n = max(SIZES)

    def some(density, empty):
        d = rng.integers(1, 128, (R, C)).astype(np.uint8)
        d[rng.uniform(size=(R, C)) >= density] = 0
        d[:, rng.uniform(size=C) < empty] = 0
        return d

    dq = np.stack([some(*((0.15, 0.4) if i % 3 == 0 else (1.0, 0.0) if i % 3 == 1 else (0.5, 0.1))) for i in range(n)])
    ddb = np.stack([some(*((0.2, 0.3) if i % 2 == 0 else (0.9, 0.05))) for i in range(n)])
    ddb[0] = np.roll(dq[0], 3, axis=1)                 # within every size: a rolled copy, a duplicate pair, a zero
    ddb[1] = 0
    for i in range(2, n, 7):
        ddb[i] = np.roll(dq[i % 5], i % C, axis=1)     # rolled copies of queries: several equal best candidates
    ddb[40] = ddb[36]                                  # duplicates: ties between candidates
    ddb[100] = ddb[3]
    dq[1] = 0
    dq[64] = dq[2]
    for a in (dq, ddb):
        a.setflags(write=False)
    return dq, ddb, handles(dq), handles(ddb)


def _limits(rng, nq, ndb):
    lim = rng.integers(0, ndb + 1, nq).astype(np.int32)
    lim[::3] = ndb
    lim[1::5] = 0
    lim[2::7] = min(1, ndb)
    return lim


@pytest.mark.parametrize("ndb", SIZES)
@pytest.mark.parametrize("nq", SIZES)
def test_sizes_top_k_and_limits(ctx, nq, ndb):
    """A query's hits are a prefix of its ranking: the checker runs once at top_k 64, the device at 1, 3 and 64."""
    R, C = 20, 60
    prm = place_params(R, C, 80.0)
    dq, ddb, uq, udb = _pool(R, C)
    lim = _limits(np.random.default_rng([13, nq, ndb]), nq, ndb)
    for limit in (None, lim):
        want = place_lib.match(dq[:nq], ddb[:ndb], 64, limit)
        assert limit is None or ndb < 64 or (want["match_idx"][:, 63] >= 0).any()
        for top_k in (1, 3, 64):
            got = match(ctx, prm, uq[:nq], udb[:ndb], top_k, limit)
            assert got.tobytes() == np.ascontiguousarray(want[:, :top_k]).tobytes(), (top_k, limit is None)


@pytest.mark.parametrize("R,C", [(4, 8), (32, 64), (21, 9), (8, 63)])
def test_other_shapes(ctx, R, C):
    prm = place_params(R, C, 30.0)
    dq, ddb, uq, udb = _pool(R, C)
    nq, ndb = 33, 65
    lim = _limits(np.random.default_rng([14, R, C]), nq, ndb)
    for limit in (None, lim):
        want = place_lib.match(dq[:nq], ddb[:ndb], 64, limit)
        for top_k in (1, 64):
            got = match(ctx, prm, uq[:nq], udb[:ndb], top_k, limit)
            assert got.tobytes() == np.ascontiguousarray(want[:, :top_k]).tobytes(), (top_k, limit is None)


def test_no_database_and_statuses(ctx):
    prm = place_params()
    dq, ddb, uq, udb = _pool(20, 60)
    got = match(ctx, prm, uq[:3], udb[:0], 2)
    assert list(got["match_idx"].ravel()) == [-1] * 6 and list(got["distance"].ravel()) == [2.0] * 6
    assert list(got["query_idx"].ravel()) == [0, 0, 1, 1, 2, 2] and not got["shift"].any() and not got["angle_guess"].any()
    for kw in (dict(top_k=0), dict(top_k=65), dict(limit=[0, 1, 4]), dict(limit=[0, -1, 1])):
        with pytest.raises(bev_amd.BevError):
            match(ctx, prm, uq[:3], udb[:3], **kw)
    with pytest.raises(bev_amd.BevError):
        match(ctx, place_params(20, 66), uq[:3], udb[:3])


def test_the_split_of_the_queries_does_not_matter(ctx):
    """one call, two calls over halves, and groups of 7 queries inside a call (BEV_PLACE_QUERY_GROUP)"""
    prm = place_params()
    dq, ddb, uq, udb = _pool(20, 60)
    nq, ndb = 65, 130
    lim = _limits(np.random.default_rng(15), nq, ndb)
    whole = match(ctx, prm, uq[:nq], udb[:ndb], 3, lim)
    halves = match(ctx, prm, uq[:nq], udb[:ndb], 3, lim, pieces=2)
    os.environ["BEV_PLACE_QUERY_GROUP"] = "7"
    try:
        groups = match(ctx, prm, uq[:nq], udb[:ndb], 3, lim)
    finally:
        del os.environ["BEV_PLACE_QUERY_GROUP"]
    assert whole.tobytes() == halves.tobytes() == groups.tobytes()
    assert whole.tobytes() == place_lib.match(dq[:nq], ddb[:ndb], 3, lim).tobytes()
