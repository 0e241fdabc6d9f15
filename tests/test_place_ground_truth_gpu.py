"""GPU: place retrieval against ground truth (tests/place_cases.py): on the world of ground_truth_cases.py the
device retrieves every query's own frame, its yaw guess is within a sector of the truth, and its hits, handed as they are to
the fine registration under the whole tool's settings, give the true yaw: the sign of the guess and the hand-over."""
import numpy as np
import pytest
import torch

import bev_amd
import place_cases
import place_lib
from bev_amd import MATCH_DTYPE, PLACE_HIT_DTYPE
from packed_cases import _dev, _p, _pack
from place_gpu_lib import HB, guarded

pytestmark = pytest.mark.gpu


def test_retrieval_and_hand_over():
    S = place_cases.case()
    prm = place_cases.params()
    n_db, n_q = len(S["db_clouds"]), len(S["q_clouds"])
    frames = S["db_clouds"] + S["q_clouds"]  # one list: a hit's indices are the registration call's frame indices
    n = len(frames)
    limit = np.full(n, n_db, np.int32)       # every frame's candidates: the database frames
    ctx = bev_amd.BevContext(_p(), device=0, max_batch=8)
    try:
        offs, flat = _pack(frames)
        d_in, d_units, d_hits = _dev(flat), guarded(n * HB), guarded(n * PLACE_HIT_DTYPE.itemsize)
        torch.cuda.synchronize()
        ctx.place_descriptor_device(n, d_in.data_ptr(), offs, 0, d_units.data_ptr(), prm)
        ctx.place_match_device(n, d_units.data_ptr(), n, d_units.data_ptr(), d_hits.data_ptr(), 1, limit, prm)
        ctx.synchronize()
        hits = d_hits[: n * PLACE_HIT_DTYPE.itemsize].cpu().numpy().view(PLACE_HIT_DTYPE)
        batch = ctx.place_retrieval_batch(frames, 1, limit, prm)[:, 0]
        assert hits.tobytes() == batch.tobytes()
        want = place_lib.match(np.stack([place_lib.descriptor([(c, None)], prm) for c in frames]),
                               np.stack([place_lib.descriptor([(c, None)], prm) for c in S["db_clouds"]]))[:, 0]
        assert hits.tobytes() == want.tobytes()
        q_hits = hits[n_db:]
        assert np.array_equal(q_hits["query_idx"], n_db + np.arange(n_q))
        assert np.array_equal(q_hits["match_idx"], S["truth"])
        for k, h in enumerate(q_hits):
            T = place_cases.gt.inverse(S["db_poses"][h["match_idx"]]) @ S["q_poses"][k]
            assert place_cases.angle_error(h["angle_guess"], place_cases.yaw_of(T)) <= place_cases.SECTOR_DEG, k
        # the first twelve bytes of a hit are a bev_match_t: the hits of the queries turned by 0 and 90 degrees, as they are
        pick = np.flatnonzero(np.isin(S["turn"], (0.0, 90.0)))
        assert len(pick) == 14
        matches = np.ascontiguousarray(q_hits[pick]).view(np.uint8).reshape(len(pick), -1)[:, :MATCH_DTYPE.itemsize].copy().view(MATCH_DTYPE).reshape(-1)
        assert np.array_equal(matches["match_idx"], S["truth"][pick])
        res = ctx.fine_registration(frames, matches, params=bev_amd.icp_whole_defaults())
        for r, k in zip(res, pick):
            T = place_cases.gt.inverse(S["db_poses"][S["truth"][k]]) @ S["q_poses"][k]
            err = place_cases.angle_error(place_cases.yaw_of(np.asarray(r["T"], np.float64).reshape(4, 4)), place_cases.yaw_of(T))
            print("query", k, "turn", S["turn"][k], "yaw error", err)
            assert err <= 1.0, k
    finally:
        ctx.close()
