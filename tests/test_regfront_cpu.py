"""CPU: the registration front end's checker (tests/regfront/regfront_oracle.c) against an independent numpy / Python
restatement of the contract in DESIGN.md "Registration front end", the closed-form 2 x 2 eigenvector against
numpy.linalg.eigh, and the ABI surface without a GPU."""
import math

import numpy as np
import pytest

import bev_amd
import regfront_lib as rl

f32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _checker():
    rl.build()


# ---- independent restatement ------------------------------------------------------------------------------------------
def _round_half_away(v):
    v = f32(v)
    t = f32(math.trunc(float(v)))
    if abs(float(v) - float(t)) >= 0.5:  # (v - t is exact in float)
        t = f32(t + f32(math.copysign(1.0, float(v))))
    return t


def py_top(cloud):
    cells = {}
    for i, p in enumerate(cloud):
        if p["label"] == 0 or not (np.isfinite(p["x"]) and np.isfinite(p["y"]) and np.isfinite(p["z"])):
            continue
        gx = _round_half_away(f32(f32(p["x"]) + f32(100.0)) / f32(20.0))
        gy = _round_half_away(f32(f32(p["y"]) + f32(100.0)) / f32(20.0))
        if not (0 <= gx < 10 and 0 <= gy < 10):
            continue
        cells.setdefault((int(gx), int(gy)), []).append(i)
    out = []
    for key in sorted(cells):
        idx = cells[key]
        if len(idx) < 20:
            continue
        k = int(_round_half_away(f32(0.2) * f32(len(idx))))
        idx = sorted(idx, key=lambda i: (-float(cloud[i]["z"]), i))
        out += [(cloud[i]["x"], cloud[i]["y"], 0.0, 0.0) for i in idx[:k]]
    return np.array(out, dtype=np.float32).reshape(-1, 4)


def py_voxel(xyz, leaf):
    xyz = np.asarray(xyz, np.float32)
    fin = [i for i in range(len(xyz)) if np.all(np.isfinite(xyz[i, :3]))]
    if not fin:
        return np.zeros((0, 4), np.float32)
    mn = [min(xyz[i, d] for i in fin) for d in range(3)]
    mx = [max(xyz[i, d] for i in fin) for d in range(3)]
    inv = f32(1.0) / f32(leaf)
    dd = [int(f32(f32(mx[d] - mn[d]) * inv)) + 1 for d in range(3)]
    if dd[0] * dd[1] * dd[2] > 2**31 - 1:
        return xyz.copy()
    minb = [int(math.floor(f32(mn[d] * inv))) for d in range(3)]
    div = [int(math.floor(f32(mx[d] * inv))) - minb[d] + 1 for d in range(3)]
    vox = {}
    for i in fin:
        ijk = [int(f32(f32(math.floor(f32(xyz[i, d] * inv))) - f32(minb[d]))) for d in range(3)]
        idx = (ijk[0] + ijk[1] * div[0] + ijk[2] * div[0] * div[1]) % 2**32
        vox.setdefault(idx, []).append(i)
    out = []
    for idx in sorted(vox):
        s = [f32(0.0)] * 3
        for i in vox[idx]:
            s = [f32(s[d] + xyz[i, d]) for d in range(3)]
        c = f32(len(vox[idx]))
        out.append([s[0] / c, s[1] / c, s[2] / c, 0.0])
    return np.array(out, dtype=np.float32)


def _closed_form(a, b, c):
    """the contract's eigenvector of the smallest eigenvalue of [[a, b], [b, c]] (float inputs, double math)"""
    h = 0.5 * (float(c) - float(a))
    s = math.sqrt(h * h + float(b) * float(b))
    if b == 0:
        v = (1.0, 0.0) if a <= c else (0.0, 1.0)
    elif h >= 0:
        v = (h + s, -float(b))
    else:
        v = (float(b), h - s)
    n = math.sqrt(v[0] * v[0] + v[1] * v[1])
    return f32(v[0] / n), f32(v[1] / n)


def py_normals(xyz, radius, vp=(0.0, 0.0)):
    xyz = np.asarray(xyz, np.float32)
    r2 = f32(float(radius) * float(radius))
    out = np.zeros((len(xyz), 8), np.float32)
    nns = []
    for q in range(len(xyz)):
        nb = []
        for j in range(len(xyz)):
            d = xyz[j, :3] - xyz[q, :3]
            if f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2]) <= r2:
                nb.append(j)
        nns.append(len(nb))
        nx = ny = nz = cv = f32(0.0)
        if len(nb) == 1:
            nx = ny = nz = cv = f32("nan")
        elif len(nb) == 2:
            vx = float(f32(xyz[nb[0], 0] - xyz[nb[1], 0]))
            vy = float(f32(xyz[nb[0], 1] - xyz[nb[1], 1]))
            norm = math.sqrt(vx * vx + vy * vy)
            with np.errstate(all="ignore"):
                nx, ny = (f32(-vy / norm), f32(vx / norm)) if norm > 0 else (f32("nan"), f32("nan"))
        elif len(nb) >= 3:
            sx = sy = f32(0.0)
            for j in nb:
                sx, sy = f32(sx + xyz[j, 0]), f32(sy + xyz[j, 1])
            mx, my = sx / f32(len(nb)), sy / f32(len(nb))
            a = b = c = f32(0.0)
            for j in nb:
                ex, ey = f32(xyz[j, 0] - mx), f32(xyz[j, 1] - my)
                a, b, c = f32(a + f32(ex * ex)), f32(b + f32(ex * ey)), f32(c + f32(ey * ey))
            nx, ny = _closed_form(a, b, c)
            with np.errstate(all="ignore"):
                cv = f32(nx / f32(f32(-ny) + nx))
        if len(nb) >= 2:
            cs = f32(float(f32(f32(vp[0]) - xyz[q, 0])) * float(nx) + float(f32(f32(vp[1]) - xyz[q, 1])) * float(ny))
            if cs < 0:
                nx, ny, nz = -nx, -ny, -nz
        out[q, 0], out[q, 1], out[q, 2], out[q, 4] = nx, ny, nz, cv
    u = out.view(np.uint32)
    u[np.isnan(out)] = 0x7FC00000
    return out, np.array(nns)


def _same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _cloud(xyz, label=1):
    c = np.zeros(len(xyz), dtype=bev_amd.POINT_DTYPE)
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    c["x"], c["y"], c["z"], c["label"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], label
    return c


# ---- top part ---------------------------------------------------------------------------------------------------------
def test_top_part_cells_of_19_and_20_points():
    rng = np.random.default_rng(1)
    a = np.c_[rng.uniform(-5, 5, 19), rng.uniform(-5, 5, 19), rng.uniform(0, 3, 19)]      # cell (5, 5): 19, skipped
    b = np.c_[rng.uniform(15, 25, 20), rng.uniform(-5, 5, 20), rng.uniform(0, 3, 20)]    # cell (6, 5): 20 -> 4 points
    c = _cloud(np.r_[a, b])
    got = rl.top_part(c)
    assert len(got) == 4
    assert _same(got, py_top(c))
    assert np.all(got[:, 2] == 0) and np.all(got[:, 3] == 0)


def test_top_part_round_not_floor_at_the_edges():
    rng = np.random.default_rng(2)
    xs = []
    for x in (89.99, 90.0, -110.0, -90.01, -109.99):
        xs.append(np.c_[np.full(25, x), rng.uniform(-5, 5, 25), rng.uniform(0, 3, 25)])
    c = _cloud(np.concatenate(xs))
    got = rl.top_part(c)
    # 89.99 -> cell 9; 90.0 -> round(9.5) = 10: dropped; -110 -> round(-0.5) = -1: dropped; -90.01 and -109.99 -> cell 0
    assert len(got) == 3 * 5
    assert not np.any(got[:, 0] == 90.0) and not np.any(got[:, 0] == -110.0)
    assert _same(got, py_top(c))


def test_top_part_equal_z_ties_across_the_selection_boundary():
    rng = np.random.default_rng(3)
    n = 40  # k = 8
    z = np.r_[np.full(6, 5.0), np.full(10, 4.0), rng.uniform(0, 3, n - 16)]
    xyz = np.c_[rng.uniform(-5, 5, n), rng.uniform(-5, 5, n), z]
    perm = rng.permutation(n)
    c = _cloud(xyz[perm])
    c["z"][c["z"] == 4.0] = np.float32(-0.0) + 4.0  # (the 4.0 group straddles rank 8)
    got = rl.top_part(c)
    assert len(got) == 8
    exp = py_top(c)
    assert _same(got, exp)
    # the two 4.0 points kept are the two lowest input indices among the 4.0 points
    four = [i for i in range(n) if c["z"][i] == 4.0][:2]
    assert _same(got[6:, :2], np.c_[c["x"][four], c["y"][four]])


def test_top_part_skips_ground_and_non_finite():
    rng = np.random.default_rng(4)
    xyz = np.c_[rng.uniform(-5, 5, 60), rng.uniform(-5, 5, 60), rng.uniform(0, 3, 60)]
    c = _cloud(xyz)
    c["label"][:10] = 0
    c["z"][10:13] = np.nan
    c["x"][13] = np.inf
    got = rl.top_part(c)
    assert len(got) == round(0.2 * 46)
    assert _same(got, py_top(c))
    assert len(rl.top_part(c[:0])) == 0


def test_top_part_random_clouds_match_the_restatement():
    rng = np.random.default_rng(5)
    for t in range(5):
        n = 3000
        xyz = np.c_[rng.uniform(-115, 95, n), rng.uniform(-115, 95, n), np.round(rng.uniform(-2, 8, n), 1)]
        c = _cloud(xyz)
        c["label"][rng.random(n) < 0.2] = 0
        assert _same(rl.top_part(c), py_top(c))


def test_max_out_bound():
    rng = np.random.default_rng(6)
    for n in (0, 19, 20, 100, 5000):
        xyz = np.c_[rng.uniform(-110, 90, n), rng.uniform(-110, 90, n), rng.uniform(0, 3, n)]
        assert len(rl.top_part(_cloud(xyz))) <= rl.lib().rf_max_out(n) == n // 5 + 51


# ---- voxel grid -------------------------------------------------------------------------------------------------------
def test_voxel_boundaries_and_negative_coordinates():
    pts = np.array([[0.0, 0.0, 0.0], [0.19999, 0.0, 0.0], [0.2, 0.0, 0.0], [-0.0001, -0.2, 0.0], [-0.2, -0.2, 0.0],
                    [-0.4, 0.4, 0.0], [0.1, 0.1, 0.0], [-1.3, 2.7, 0.0], [-1.3, 2.7, 0.0]], np.float32)
    got, info = rl.voxel(pts, 0.2, want_info=True)
    assert info[0] == 0 and len(got) < len(pts)  # multi-point voxels
    assert _same(got, py_voxel(rl._xyz4(pts), 0.2))


def test_voxel_random_3d_and_order():
    rng = np.random.default_rng(7)
    for t in range(4):
        pts = np.c_[rng.uniform(-3, 3, 800), rng.uniform(-3, 3, 800), rng.uniform(-1, 1, 800) * (t % 2)].astype(np.float32)
        got = rl.voxel(pts, 0.25)
        assert _same(got, py_voxel(rl._xyz4(pts), 0.25))


def test_voxel_overflow_returns_the_input():
    pts = np.array([[-1000.0, -1000.0, 0.0], [1000.0, 1000.0, 0.0], [0.0, 0.0, 5.0], [3.0, 3.0, 3.0]], np.float32)
    got, info = rl.voxel(pts, 0.001, want_info=True)
    assert info[0] == 1
    assert _same(got, rl._xyz4(pts))
    assert _same(got, py_voxel(rl._xyz4(pts), 0.001))


def test_voxel_drops_non_finite_points_and_empty():
    pts = np.array([[0.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [0.05, 0.05, 0.0], [np.inf, 1, 1]], np.float32)
    got = rl.voxel(pts, 0.2)
    assert len(got) == 1
    assert _same(got, py_voxel(rl._xyz4(pts), 0.2))
    assert len(rl.voxel(np.zeros((0, 4), np.float32), 0.2)) == 0


# ---- normals ----------------------------------------------------------------------------------------------------------
def test_normals_neighbour_counts_1_2_3_and_coincident():
    pts = np.array([
        [50.0, 50.0, 0.0],                                            # |N| = 1
        [10.0, 10.0, 0.0], [11.0, 10.5, 0.0],                         # |N| = 2
        [-10.0, 0.0, 0.0], [-9.5, 0.3, 0.0], [-9.0, 0.1, 0.0], [-10.2, -0.4, 0.0],  # |N| >= 3
        [30.0, -30.0, 0.0], [30.0, -30.0, 0.0],                       # |N| = 2, coincident: NaN
        [-30.0, 30.0, 0.0], [-30.0, 30.0, 0.0], [-30.0, 30.0, 0.0],   # |N| = 3, coincident: b == 0, a == c
        [0.0, -40.0, 0.0], [1.0, -40.0, 0.0], [2.0, -40.0, 0.0],      # a line along x: b == 0
    ], np.float32)
    got, nn = rl.normals(pts, 2.0, want_nn=True)
    exp, enn = py_normals(rl._xyz4(pts), 2.0)
    assert list(nn) == list(enn)
    assert {1, 2, 3, 4} <= set(nn.tolist())
    assert _same(got, exp)
    u = got.view(np.uint32)
    assert np.all(u[0, [0, 1, 2, 4]] == 0x7FC00000)                  # |N| = 1: NaN (canonical)
    assert np.all(u[7:9, [0, 1]] == 0x7FC00000)                        # coincident pair
    assert np.all(got[[9, 10, 11], 0] == 1.0) and np.all(got[[9, 10, 11], 1] == 0.0)  # a == c: (1, 0)
    assert np.all(np.abs(got[12:15, 1]) == 1.0) and np.all(got[12:15, 4] == 0.0 * 0 + got[12:15, 4])
    assert np.all(u[:, [3, 5, 6, 7]] == 0)


def test_normals_random_match_the_restatement():
    rng = np.random.default_rng(8)
    for t in range(3):
        pts = np.c_[rng.uniform(-6, 6, 300), rng.uniform(-6, 6, 300), np.zeros(300)].astype(np.float32)
        vp = (float(rng.uniform(-5, 5)), float(rng.uniform(-5, 5)), 0.0)
        got = rl.normals(pts, 1.5, vp)
        exp, _ = py_normals(rl._xyz4(pts), 1.5, vp[:2])
        assert _same(got, exp)


def test_closed_form_against_eigh():
    rng = np.random.default_rng(9)
    checked = 0
    for t in range(3000):
        a, c = f32(rng.uniform(0, 10)), f32(rng.uniform(0, 10))
        b = f32(rng.uniform(-5, 5)) if t % 10 else f32(0.0)
        w, v = np.linalg.eigh(np.array([[a, b], [b, c]], np.float64))
        nx, ny = _closed_form(a, b, c)
        if w[1] - w[0] < 1e-3 * max(1.0, abs(w[1])):
            continue
        ang = math.asin(min(1.0, abs(float(nx) * v[1, 0] - float(ny) * v[0, 0])))  # (sin: well conditioned near 0)
        assert ang <= 1e-6, (a, b, c, ang)
        checked += 1
    assert checked > 2500
    # b == 0 and a == c are exact
    assert _closed_form(f32(1), f32(0), f32(2)) == (1.0, 0.0)
    assert _closed_form(f32(2), f32(0), f32(1)) == (0.0, 1.0)
    assert _closed_form(f32(3), f32(0), f32(3)) == (1.0, 0.0)


def test_chain_is_the_three_steps():
    rng = np.random.default_rng(10)
    n = 4000
    xyz = np.c_[rng.normal(0, 15, n), rng.normal(0, 15, n), rng.uniform(-1, 6, n)]
    c = _cloud(xyz)
    got = rl.chain(c)
    vox = rl.voxel(rl.top_part(c), 0.2)
    nrm = rl.normals(vox, 2.0)
    assert len(got) == len(vox) > 0
    assert _same(got[:, :4], vox) and _same(got[:, 4:8], nrm[:, :4]) and _same(got[:, 8], nrm[:, 4])
    assert np.all(got[:, 9:] == 0)


# ---- ABI without a GPU ------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["bev_top_part_flatten", "bev_voxel_grid_xyz", "bev_normals_2d", "bev_registration_front_device_resident",
               "bev_regfront_max_out"]


def test_new_symbols_are_exported():
    lib = bev_amd.load_lib()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s) and s in bev_amd.ABI_SYMBOLS


def test_max_out_needs_no_gpu():
    assert bev_amd.regfront_max_out(0) == 51
    assert bev_amd.regfront_max_out(133312) == 133312 // 5 + 51
    assert bev_amd.regfront_max_out(10**9) == 10**9 // 5 + 51


def test_new_entries_fail_loudly_without_a_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    lib = bev_amd.load_lib()
    # a null context is an argument error, not a crash
    assert lib.bev_top_part_flatten(None, None, 0, None, None) == -1
    assert lib.bev_registration_front_device_resident(None, 1, None, None, 0.2, 2.0, None, None, 0, None) == -1
    with pytest.raises(bev_amd.BevError, match="no usable HIP device"):
        bev_amd.BevContext(bev_amd.params_for_sensor("HDL_64E"), device=0, max_batch=1, max_points=1000)
