"""What the GPU tests of place retrieval share: one descriptor call and one match call on device buffers
with guards behind every output, and the checker's side of both.  Tests only."""
from __future__ import annotations

import numpy as np
import torch

import bev_amd
import place_lib
from bev_amd import PLACE_HIT_DTYPE
from packed_cases import GUARD, PATTERN, _dev, _pack

HB = place_lib.HANDLE_BYTES


def guarded(n_bytes):
    return torch.full((n_bytes + GUARD,), PATTERN, dtype=torch.uint8, device=torch.device("cuda:0"))


def guard_ok(t, n_bytes):
    return bool((t[n_bytes:] == PATTERN).all())


def descriptors(ctx, frames, prm, maps=None, want_desc=True, want_units=True):
    """One bev_place_descriptor_device_resident call: (desc (n, R, C) uint8 or None, units (n, HB) uint8 or None), the guards
    checked.  maps: None, or (map_offsets, entry_frame, entry_pose)."""
    offs, flat = _pack(frames)
    n = len(frames) if maps is None else len(maps[0]) - 1
    cells = prm.n_rings * prm.n_sectors
    d_in, d_desc, d_units = _dev(flat), guarded(n * cells), guarded(n * HB)
    torch.cuda.synchronize()
    kw = {} if maps is None else dict(map_offsets=maps[0], entry_frame=maps[1], entry_pose=maps[2])
    ctx.place_descriptor_device(len(frames), d_in.data_ptr(), offs, d_desc.data_ptr() if want_desc else 0,
                                d_units.data_ptr() if want_units else 0, prm, **kw)
    ctx.synchronize()
    assert guard_ok(d_desc, n * cells if want_desc else 0) and guard_ok(d_units, n * HB if want_units else 0)
    return (d_desc[: n * cells].cpu().numpy().reshape(n, prm.n_rings, prm.n_sectors) if want_desc else None,
            d_units[: n * HB].cpu().numpy().reshape(n, HB) if want_units else None)


def handles(descs) -> np.ndarray:
    """the checker's records of (n, R, C) descriptors: (n, HB) uint8"""
    return np.stack([place_lib.handle(d) for d in descs]) if len(descs) else np.zeros((0, HB), np.uint8)


def match(ctx, prm, units_q, units_db, top_k=1, limit=None, pieces=None):
    """bev_place_match_device_resident on uploaded records: (n_queries, top_k) hits, the guard checked.  pieces: the queries
    go in that many calls over consecutive parts (a hit's query_idx then counts within its call)."""
    nq, ndb = len(units_q), len(units_db)
    dq, ddb = _dev(units_q) if nq else guarded(0), _dev(units_db) if ndb else guarded(0)
    n_bytes = nq * top_k * PLACE_HIT_DTYPE.itemsize
    d_hits = guarded(n_bytes)
    torch.cuda.synchronize()
    cuts = [0, nq] if pieces is None else [nq * i // pieces for i in range(pieces + 1)]
    for a, b in zip(cuts[:-1], cuts[1:]):
        ctx.place_match_device(b - a, dq.data_ptr() + a * HB, ndb, ddb.data_ptr() if ndb else 0,
                               d_hits.data_ptr() + a * top_k * PLACE_HIT_DTYPE.itemsize, top_k,
                               None if limit is None else np.asarray(limit, np.int32)[a:b], prm)
    ctx.synchronize()
    assert guard_ok(d_hits, n_bytes)
    hits = d_hits[:n_bytes].cpu().numpy().view(PLACE_HIT_DTYPE).reshape(nq, top_k).copy()
    for a, b in zip(cuts[:-1], cuts[1:]):
        hits["query_idx"][a:b] += a
    return hits
