"""The plain reference of the registration stages: brute-force nearest neighbours, point-to-point ICP by the
rigid least-squares motion (np.linalg.svd) and point-to-plane ICP by the linearised normal equations (np.linalg.solve), the
tools' yaw guesses and their report arithmetic.  numpy only, nothing shared with the checkers (icp_lib, fineicp_lib, the
*_cases.py compositions, oracle_lib): it restates the mathematics, not the contract's float32 associations.  Every function
takes dtype=np.float64; dtype=np.float32 runs the same plain code in float32 (the spread between the two sets the tests'
tolerance).  Stopping criteria are not modelled: the loops run a fixed number of iterations.  Tests only."""
from __future__ import annotations

import numpy as np

CHUNK = 32     # rows of cur at a time: the block of distances stays in cache


def nearest(cur, tgt, dtype=np.float64):
    """(index int64, squared distance) of every row of cur (n, 3) in tgt (m, 3), brute force in chunks of rows; the first
    index on equal distance; a target row with a non-finite coordinate is never returned.  Index -1 and distance inf where
    there is no finite target or the row of cur is not finite."""
    cur = np.asarray(cur, dtype).reshape(-1, 3)
    tgt = np.asarray(tgt, dtype).reshape(-1, 3)
    ok = np.flatnonzero(np.isfinite(tgt).all(axis=1))
    idx = np.full(len(cur), -1, np.int64)
    d2 = np.full(len(cur), np.inf, dtype)
    if not len(ok) or not len(cur):
        return idx, d2
    t = tgt[ok]
    for a in range(0, len(cur), CHUNK):
        c = cur[a: a + CHUNK]
        with np.errstate(invalid="ignore", over="ignore"):
            d = (c[:, 0, None] - t[None, :, 0]) ** 2
            d += (c[:, 1, None] - t[None, :, 1]) ** 2
            d += (c[:, 2, None] - t[None, :, 2]) ** 2
        d[~np.isfinite(d)] = np.inf
        k = d.argmin(axis=1)
        best = d[np.arange(len(c)), k]
        found = np.isfinite(best)
        idx[a: a + CHUNK] = np.where(found, ok[k], -1)
        d2[a: a + CHUNK] = best
    return idx, d2


def apply(T, pts, dtype=np.float64):
    """R p + t of every row"""
    T = np.asarray(T, dtype).reshape(4, 4)
    return np.asarray(pts, dtype).reshape(-1, 3) @ T[:3, :3].T + T[:3, 3]


def rigid_fit(s, t, dtype=np.float64):
    """the rigid motion (4 x 4) that takes the rows of s onto the rows of t in the least-squares sense: centroids, the SVD of
    the 3 x 3 cross-covariance, the determinant fix"""
    s, t = np.asarray(s, dtype), np.asarray(t, dtype)
    cs, ct = s.mean(axis=0), t.mean(axis=0)
    H = (t - ct).T @ (s - cs)
    U, _, Vt = np.linalg.svd(H)
    S = np.eye(3, dtype=dtype)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1
    R = U @ S @ Vt
    T = np.eye(4, dtype=dtype)
    T[:3, :3] = R
    T[:3, 3] = ct - R @ cs
    return T


def plane_fit(s, t, n, dtype=np.float64):
    """the linearised point-to-plane step: rows [s x n, n], right side n . (t - s), the 6 x 6 normal equations solved, the
    increment Rz(gamma) Ry(beta) Rx(alpha) plus the translation"""
    s, t, n = (np.asarray(a, dtype) for a in (s, t, n))
    A = np.concatenate([np.cross(s, n), n], axis=1)
    b = (n * (t - s)).sum(axis=1)
    x = np.linalg.solve(A.T @ A, A.T @ b)
    al, be, ga = x[0], x[1], x[2]
    rx = np.array([[1, 0, 0], [0, np.cos(al), -np.sin(al)], [0, np.sin(al), np.cos(al)]], dtype)
    ry = np.array([[np.cos(be), 0, np.sin(be)], [0, 1, 0], [-np.sin(be), 0, np.cos(be)]], dtype)
    rz = np.array([[np.cos(ga), -np.sin(ga), 0], [np.sin(ga), np.cos(ga), 0], [0, 0, 1]], dtype)
    T = np.eye(4, dtype=dtype)
    T[:3, :3] = rz @ ry @ rx
    T[:3, 3] = x[3:]
    return T


def _loop(src, tgt, guess, D, iterations, step, dtype, trace):
    src = np.asarray(src, dtype).reshape(-1, 3)
    tgt = np.asarray(tgt, dtype).reshape(-1, 3)
    T = np.asarray(guess, dtype).reshape(4, 4).copy()
    out = []
    for _ in range(int(iterations)):
        cur = apply(T, src, dtype)
        idx, d2 = nearest(cur, tgt, dtype)
        keep = (idx >= 0) & (d2 <= dtype(D) * dtype(D))
        if trace is not None:
            trace.append((T.copy(), idx.copy(), d2.copy(), keep.copy()))
        T = (step(cur[keep], idx[keep]) @ T).astype(dtype)
        out.append(T.copy())
    return out


def point_to_point(src, tgt, guess, D, iterations, dtype=np.float64, trace=None):
    """[T after iteration 1, ..., T after `iterations`] (4 x 4 each, source to target): per iteration the source under the
    running T, its nearest neighbours, the pairs with d^2 <= D^2, their rigid least-squares motion T_i, T = T_i T.  Iterate
    k is what max_iterations = k gives.  trace: a list that receives (T before, index, d^2, kept) per iteration."""
    tgt = np.asarray(tgt, dtype).reshape(-1, 3)
    return _loop(src, tgt, guess, D, iterations, lambda c, i: rigid_fit(c, tgt[i], dtype), dtype, trace)


def point_to_plane(src, tgt, tgt_normals, guess, D, iterations, dtype=np.float64, trace=None):
    """the same loop with the linearised point-to-plane step against the target's normals"""
    tgt = np.asarray(tgt, dtype).reshape(-1, 3)
    nrm = np.asarray(tgt_normals, dtype).reshape(-1, 3)
    return _loop(src, tgt, guess, D, iterations, lambda c, i: plane_fit(c, tgt[i], nrm[i], dtype), dtype, trace)


def fitness(src, tgt, T, dtype=np.float64):
    """the mean squared distance of the source under T to its nearest neighbours, no distance limit"""
    _, d2 = nearest(apply(T, src, dtype), tgt, dtype)
    d2 = d2[np.isfinite(d2)]
    return float(d2.mean()) if len(d2) else np.finfo(np.float64).max


def yaw_guess(theta_deg, which, dtype=np.float64):
    """the tools' start matrices (include/bev_mi355x.h): a yaw about z by theta (which 0) or by theta + 180 (which 1), theta
    the match's float angle_guess"""
    th = np.float32(theta_deg) + (np.float32(180.0) if which else np.float32(0.0))
    rad = float(th) / 180.0 * np.pi
    T = np.eye(4, dtype=dtype)
    T[0, 0] = T[1, 1] = np.cos(rad)
    T[0, 1], T[1, 0] = -np.sin(rad), np.sin(rad)
    return T


def report(T, T_guess, dtype=np.float64):
    """(diff_xy, diff_yaw in degrees) of the tools' report line (Bookkeeping): the planar distance of the two
    translations, and the angle about z of R^-1 R_guess, atan2(r10, r00), wrapped once into +-180"""
    T = np.asarray(T, dtype).reshape(4, 4)
    G = np.asarray(T_guess, dtype).reshape(4, 4)
    xy = np.hypot(T[0, 3] - G[0, 3], T[1, 3] - G[1, 3])
    rel = np.linalg.inv(T[:3, :3]) @ G[:3, :3]
    yaw = np.degrees(np.arctan2(rel[1, 0], rel[0, 0]))
    if yaw > 180.0:
        yaw -= 360.0
    if yaw < -180.0:
        yaw += 360.0
    return float(xy), float(yaw)
