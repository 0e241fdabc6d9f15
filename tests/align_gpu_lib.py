"""What the GPU tests of the translation guess of retrieved pairs share: one grid call and one hits call on
device buffers with guards behind every output, and the checker's side of both.  Tests only."""
from __future__ import annotations

import numpy as np
import torch

import align_lib
from bev_amd import ALIGN_DETAIL_DTYPE, ICP_RESULT_DTYPE, MATCH_DTYPE
from packed_cases import GUARD, PATTERN, _dev, _pack

R, D = ICP_RESULT_DTYPE.itemsize, ALIGN_DETAIL_DTYPE.itemsize


def guarded(n_bytes):
    return torch.full((n_bytes + GUARD,), PATTERN, dtype=torch.uint8, device=torch.device("cuda:0"))


def guard_ok(t, n_bytes):
    return bool((t[n_bytes:] == PATTERN).all())


def grids(ctx, frames, prm, maps=None):
    """One bev_align_grid_device_resident call: (grids (n, G, G) uint8, energy (n,) uint32), the guards checked.  maps: None, or
    (map_offsets, entry_frame, entry_pose)."""
    offs, flat = _pack(frames)
    n = len(frames) if maps is None else len(maps[0]) - 1
    cells = prm.grid * prm.grid
    d_in, d_grids, d_energy = _dev(flat), guarded(n * cells), guarded(n * 4)
    torch.cuda.synchronize()
    kw = {} if maps is None else dict(map_offsets=maps[0], entry_frame=maps[1], entry_pose=maps[2])
    ctx.align_grid_device(len(frames), d_in.data_ptr(), offs, d_grids.data_ptr(), d_energy.data_ptr(), prm, **kw)
    ctx.synchronize()
    assert guard_ok(d_grids, n * cells) and guard_ok(d_energy, n * 4)
    return (d_grids[: n * cells].cpu().numpy().reshape(n, prm.grid, prm.grid),
            d_energy[: n * 4].cpu().numpy().view(np.uint32).copy())


def checker_grids(frames, prm, maps=None, l2g=2.0):
    if maps is None:
        return np.stack([align_lib.grid([(f, None)], prm, l2g) for f in frames])
    offs, ef, ep = maps
    return np.stack([align_lib.grid([(frames[ef[e]], ep[e]) for e in range(int(offs[g]), int(offs[g + 1]))], prm, l2g)
                     for g in range(len(offs) - 1)])


def hits(ctx, queries, cand_grids, hit_list, prm, pieces=None, want_detail=True):
    """bev_align_hits_device_resident on uploaded queries and candidate grids ((n_db, G, G) uint8; their sums of squares are
    taken from them): (results (n, 2), best (n,), detail (n, 2) or None), the guards checked.  pieces: the hits go in that many
    calls over consecutive parts."""
    m = np.ascontiguousarray(hit_list, dtype=MATCH_DTYPE)
    n, n_db = len(m), len(cand_grids)
    offs, flat = _pack(queries)
    energy = np.array([(g.astype(np.int64) ** 2).sum() for g in cand_grids], np.uint32)
    d_in = _dev(flat)
    d_grids = _dev(np.ascontiguousarray(cand_grids, np.uint8)) if n_db else guarded(0)
    d_energy = _dev(energy) if n_db else guarded(0)
    d_res, d_best, d_det = guarded(2 * n * R), guarded(4 * n), guarded(2 * n * D)
    torch.cuda.synchronize()
    cuts = [0, n] if pieces is None else [n * i // pieces for i in range(pieces + 1)]
    for a, b in zip(cuts[:-1], cuts[1:]):
        ctx.align_hits_device(len(queries), d_in.data_ptr(), offs, n_db, d_grids.data_ptr() if n_db else 0,
                              d_energy.data_ptr() if n_db else 0, m[a:b], d_res.data_ptr() + 2 * a * R, d_best.data_ptr() + 4 * a,
                              d_det.data_ptr() + 2 * a * D if want_detail else 0, prm)
    ctx.synchronize()
    assert guard_ok(d_res, 2 * n * R) and guard_ok(d_best, 4 * n) and guard_ok(d_det, 2 * n * D if want_detail else 0)
    return (d_res[: 2 * n * R].cpu().numpy().view(ICP_RESULT_DTYPE).reshape(n, 2).copy(),
            d_best[: 4 * n].cpu().numpy().view(np.int32).copy(),
            d_det[: 2 * n * D].cpu().numpy().view(ALIGN_DETAIL_DTYPE).reshape(n, 2).copy() if want_detail else None)
