"""The posed and submap rasters against a float64 world (test_raster_world_cpu.py, test_raster_world_gpu.py,
test_cli_raster_world_gpu.py): the world and the seven entry poses of ground_truth_cases.py, seen as frames with labels, put
together as maps under general rigid matrices, and a plain float64 reference that rasters WORLD coordinates.  numpy only;
nothing here comes from the oracle, the Python restatement or bev_exact.h: the contract is restated from include/bev_mi355x.h
and DESIGN.md §6f, §6g, §6i, §6j.

Frames.  Frame f is what lies within RANGE of P_f (the pose as a pose file holds it: float32 entries), as P_f^-1 p rounded to
float32, in a seeded random order.

The world is ground_truth_cases.world() — the ground at z = -1.7 and nine walls — with posts and lamps added: single points
on two jittered lattices, posts 0 to 1.8 m up, lamps 2 to 3.5 m.  The ground lies below layer 0, it is 0 or 1 in the uint8
image, and two wall records share a byte of the 24-layer image, so that world alone gives several mutants little to change
at 2 m cells; a post or a lamp is the highest point of its cell, at a height of its own, and alone in its layer.  A tenth of each frame's records has label 0: first every lamp it sees (one class of objects, as a ground marker
gives one class label 0; label 0 in EVERY frame that sees them: such a point is missing from a map), then seeded picks of
the frame's own (label 0 in SOME entries only: such a point is still in the map, from another entry).

Maps.  A map is a list of entries (frame, origin): the entry's matrix is origin^-1 P_frame, and the reference puts the world
point p at origin^-1 p.  Every map but D has one origin.
  A   frames 0 .. 4 about P_2          B   frames 6 .. 2 (descending) about P_4          C   frame 3 under the identity
  K   frames 1 .. 5 about P_3 (with A and B: what the submap tools make of key frames 2, 3, 4 at half window 2)
  T   frames 1 .. 5 about P_v = P_3 * (12 deg roll, -9 deg pitch, 5 deg yaw, a step of 6.5 m): all 12 entries of every
      matrix far from 0 and 1
  F, G  T's frames about P_v shifted along its own x by FAR_SHIFT: far origins.  (A rigid shift cannot push a map of 52 m
      off both sides of an image 224 m wide: F leaves on the low side of x, G on the high side.)  The shift is a multiple
      of 2 m, so F and G have P_v's bin, layer and height edges and cost the filter nothing.
  D   frame 3 twice: under the identity and about P_v shifted by D_SHIFT (P_v's edges again)
Posed grid (f, k) is frame f alone about POSED_ORIGINS[k]: P_2, P_v, F's origin.  CLI_POSES are the rows of a pose file of
batch_posed_bev_gen (tx ty tz yaw_deg, the only form that tool reads), applied to frame 3: the origin is P_3 M^-1.

The filter.  A float32 implementation may put a point that lies on an edge on either side.  Per configuration, a world point
is dropped from every frame if in ANY compared map or grid it lies within MARGIN of an x or y bin edge (R = 112 and R = 100),
of a layer edge or of a height step.  MARGIN is derived, not measured: a frame's coordinates stay below 64 m and those on an
image below 128 m, so one float32 rounding is at most 3.8e-6 m; the frame's own rounding, the rounding of the matrix entries times the coordinates (3 * 6e-8 * 64), three
sums per row and the tools' own evaluation of the relative pose and of sinf / cosf add up to less than 5e-5 m; 1e-3 m leaves
20 times that.  Tests only."""
from __future__ import annotations

import functools

import numpy as np

import ground_truth_cases as gt
from bev_amd import POINT_DTYPE

F32, F64 = np.float32, np.float64
MARGIN = 1e-3
RANGE = 18.0
FACTOR, CAP = 8.0, 1e-4                       # tol = FACTOR * (float32 against float64 of the plain reference), at most CAP
N_FRAMES = 7
SEED = 20271
LAMP_SPACING, POST_SPACING, OWN = 2.4, 2.2, 12   # the lattices of the lamps and posts; a frame's own picks of label 0: at least OWN
FAR_SHIFT = (96.0, -108.0)                   # F's and G's, multiples of 2 m
D_SHIFT = (-12.0, 8.0)                       # D's second origin: P_v shifted in its own x and y, multiples of 2 m

N_LAYERS, LIDAR_TO_GROUND, R_MAIN, R_FLOAT = 24, 2.0, 112.0, 100.0
# sensor: (height_res of bev_params_for_sensor, the interval the sensor is tested at)
CONFIGS = {"HDL_64E": (0.25, 1.0), "HDL_32E": (0.5, 0.5), "OS1_64": (1.0, 2.0)}
MULTI_ENTRY = ("A", "B", "K", "T", "F", "G", "D")
CLI_POSES = ((3.7, -5.3, 1.0, 33.3), (-41.2, 17.9, -1.0, 200.6))   # tz in whole metres: P_3's layer and height edges
IDENTITY12 = np.eye(3, 4, dtype=F32).reshape(12)


def yaw_translate(tx, ty, tz, yaw_deg) -> np.ndarray:
    """the pose of a batch_posed_bev_gen row in float64: a rotation about z by yaw_deg, then the translation"""
    return gt.pose(0.0, 0.0, yaw_deg, [tx, ty, tz])


@functools.lru_cache(maxsize=None)
def origins():
    """the poses of the entries and the virtual origins, float64 4 x 4 (sensor to world)"""
    P = [np.array(p) for p in gt.setup(round_poses=True)["poses"][:N_FRAMES]]
    Pv = P[3] @ gt.pose(12.0, -9.0, 5.0, [5.3, -3.7, -0.8])
    shift = lambda d, dy=0.0: Pv @ gt.pose(0, 0, 0, [d, dy, 0.0])
    cli = [P[3] @ gt.inverse(yaw_translate(*row)) for row in CLI_POSES]
    return dict(P=P, Pv=Pv, OF=shift(FAR_SHIFT[0]), OG=shift(FAR_SHIFT[1]), OD=shift(*D_SHIFT), cli=cli)


@functools.lru_cache(maxsize=None)
def maps():
    """{name: [(frame, origin)]}: the submaps, the posed grids ("posed", f, k) and the CLI's grids ("cli", k)"""
    o = origins()
    P, Pv = o["P"], o["Pv"]
    m = {"A": [(j, P[2]) for j in range(5)],
         "B": [(j, P[4]) for j in (6, 5, 4, 3, 2)],
         "C": [(3, P[3])],
         "K": [(j, P[3]) for j in range(1, 6)],
         "T": [(j, Pv) for j in range(1, 6)],
         "F": [(j, o["OF"]) for j in (5, 4, 3, 2, 1)],
         "G": [(j, o["OG"]) for j in range(1, 6)],
         "D": [(3, P[3]), (3, o["OD"])]}
    for f in range(N_FRAMES):
        for k, O in enumerate(posed_origins()):
            m["posed", f, k] = [(f, O)]
    for k, O in enumerate(o["cli"]):
        m["cli", k] = [(3, O)]
    return m


def posed_origins():
    o = origins()
    return (o["P"][2], o["Pv"], o["OF"])


SUBMAPS = ("A", "B", "C", "K", "T", "F", "G", "D")


@functools.lru_cache(maxsize=None)
def world():
    """(xyz (n, 3) float64, is_lamp (n,) bool): ground_truth_cases.world(), then the posts, then the lamps"""
    base = gt.world()[0]
    rng = np.random.default_rng([SEED, 1])
    gx, gy = np.meshgrid(np.arange(-33.0, 58.0, LAMP_SPACING), np.arange(-22.0, 22.5, LAMP_SPACING), indexing="ij")
    lamps = np.c_[gx.ravel(), gy.ravel(), np.zeros(gx.size)]
    lamps[:, :2] += rng.uniform(-0.3, 0.3, (len(lamps), 2)) * LAMP_SPACING
    lamps[:, 2] = rng.uniform(2.0, 3.5, len(lamps))
    px, py = np.meshgrid(np.arange(-33.5, 58.0, POST_SPACING), np.arange(-21.5, 22.5, POST_SPACING), indexing="ij")
    posts = np.c_[px.ravel(), py.ravel(), np.zeros(px.size)]
    posts[:, :2] += rng.uniform(-0.3, 0.3, (len(posts), 2)) * POST_SPACING
    posts[:, 2] = rng.uniform(0.0, 1.8, len(posts))
    return np.concatenate([base, posts, lamps]), np.r_[np.zeros(len(base) + len(posts), bool), np.ones(len(lamps), bool)]


@functools.lru_cache(maxsize=None)
def sightings():
    """(ids, labels) per frame before the filter: the world indices within RANGE of P_f in a seeded random order, and each
    record's label (1, or 0 for a tenth of them)"""
    xyz, is_lamp = world()
    rng = np.random.default_rng(SEED)
    ids, labels = [], []
    for P in origins()["P"]:
        seen = np.flatnonzero(np.linalg.norm(xyz - P[:3, 3], axis=1) < RANGE)
        seen = seen[rng.permutation(len(seen))]
        tenth = len(seen) // 10
        first = np.flatnonzero(is_lamp[seen])
        assert len(first) <= tenth - OWN, "the lamps alone fill a frame's tenth: no room for labels of the frame's own"
        rest = rng.permutation(np.flatnonzero(~is_lamp[seen]))
        zero = np.r_[first, rest[:tenth - len(first)]]
        lab = np.ones(len(seen), np.int16)
        lab[zero] = 0
        ids.append(seen), labels.append(lab)
    return ids, labels


def to_frame(O, xyz, dtype=F64) -> np.ndarray:
    """O^-1 p for the rows of xyz; dtype float32: the same plain code with every operand and operation in float32"""
    inv = gt.inverse(O)
    R, t = inv[:3, :3].astype(dtype), inv[:3, 3].astype(dtype)
    x = np.asarray(xyz).astype(dtype)
    return (x[:, 0, None] * R[None, :, 0] + x[:, 1, None] * R[None, :, 1] + x[:, 2, None] * R[None, :, 2] + t[None]).astype(dtype)


def near_edge(q, height_res, interval) -> np.ndarray:
    """per row of q (n, 3) float64: within MARGIN of an x or y bin edge (either range), a layer edge or a height step"""
    bad = np.zeros(len(q), bool)
    for R in (R_MAIN, R_FLOAT):
        v = (q[:, :2] + R) / interval
        bad |= (np.abs(v - np.round(v)) * interval < MARGIN).any(axis=1)
    u = q[:, 2] / height_res + LIDAR_TO_GROUND - 0.5                 # a layer edge is a half-integer of z / height_res + 2
    bad |= np.abs(u - np.round(u)) * height_res < MARGIN
    w = (q[:, 2] + LIDAR_TO_GROUND) * 4.0
    bad |= np.abs(w - np.round(w)) / 4.0 < MARGIN
    return bad


@functools.lru_cache(maxsize=None)
def dropped(sensor) -> np.ndarray:
    """bool per world point: dropped from every frame under this configuration"""
    height_res, interval = CONFIGS[sensor]
    xyz = world()[0]
    ids, _ = sightings()
    out = np.zeros(len(xyz), bool)
    by_origin = {}
    for entries in maps().values():
        for f, O in entries:
            by_origin.setdefault(id(O), (O, set()))[1].add(f)
    for O, frames in by_origin.values():
        seen = np.unique(np.concatenate([ids[f] for f in sorted(frames)]))
        out[seen[near_edge(to_frame(O, xyz[seen]), height_res, interval)]] = True
    return out


class Case:
    """One configuration: the filtered frames and what is compared."""

    def __init__(self, sensor):
        self.sensor = sensor
        self.height_res, self.interval = CONFIGS[sensor]
        self.M = int(2 * R_MAIN / self.interval)
        self.Mf = int(200.0 / self.interval + 1)
        self.xyz = world()[0]
        self.P = origins()["P"]
        self.maps = maps()
        self.drop = dropped(sensor)
        raw_ids, raw_labels = sightings()
        self.ids, self.labels, self.frames = [], [], []
        for f in range(N_FRAMES):
            keep = ~self.drop[raw_ids[f]]
            ids, lab = raw_ids[f][keep], raw_labels[f][keep]
            local = to_frame(self.P[f], self.xyz[ids]).astype(F32)
            c = np.zeros(len(ids), POINT_DTYPE)
            c["x"], c["y"], c["z"] = local[:, 0], local[:, 1], local[:, 2]
            c["intensity"], c["label"] = 1.0, lab
            c.setflags(write=False)
            self.ids.append(ids), self.labels.append(lab), self.frames.append(c)
        self.seen = np.unique(np.concatenate(raw_ids))

    # ---- what the calls are given --------------------------------------------------------------------------------------------
    def matrix(self, f, O) -> np.ndarray:
        """origin^-1 P_f as the calls take it: a row-major 3 x 4 in float32; a frame about its own pose: the exact identity"""
        return IDENTITY12 if O is self.P[f] else (gt.inverse(O) @ self.P[f])[:3].astype(F32).reshape(12)

    def entries(self, name):
        """[(frame, matrix (12,) float32)] of a map"""
        return [(f, self.matrix(f, O)) for f, O in self.maps[name]]

    def posed_matrices(self) -> np.ndarray:
        """(N_FRAMES, 3, 12) float32: frame f about POSED_ORIGINS[k]"""
        return np.stack([np.stack([self.matrix(f, O) for O in posed_origins()]) for f in range(N_FRAMES)])

    # ---- the reference -------------------------------------------------------------------------------------------------------
    def points(self, name, skip_label0=True, dtype=F64, keep_dropped=False) -> np.ndarray:
        """(n, 3): the world points the map's entries see with a non-zero label (skip_label0) or at all, the union over the
        entries of one origin, in the map's frame"""
        raw_ids, raw_labels = sightings()
        groups = {}
        for f, O in self.maps[name]:
            ids, lab = (raw_ids[f], raw_labels[f]) if keep_dropped else (self.ids[f], self.labels[f])
            groups.setdefault(id(O), (O, []))[1].append(ids[lab != 0] if skip_label0 else ids)
        return np.concatenate([to_frame(O, self.xyz[np.unique(np.concatenate(parts))], dtype) for O, parts in groups.values()])

    def reference(self, name, dtype=F64, keep_dropped=False):
        """(multi (24, M, M) uint8, single (M, M) uint8) of a map"""
        return main_images(self.points(name, True, dtype, keep_dropped), self.height_res, self.interval, dtype)

    def reference_float(self, name, skip_label0=True, dtype=F64) -> np.ndarray:
        return float_grid(self.points(name, skip_label0, dtype), self.interval, dtype)

    @functools.lru_cache(maxsize=None)
    def tol(self) -> float:
        """FACTOR times the largest difference, over every compared float grid, between the reference's plain code in float32
        and in float64; the two must agree on which cells are occupied"""
        worst = 0.0
        for name in self.maps:
            for skip in (True, False):
                a, b = self.reference_float(name, skip, F64), self.reference_float(name, skip, F32)
                assert np.array_equal(a > 0, b > 0), (name, skip)
                worst = max(worst, float(np.abs(a - b.astype(F64)).max()))
        return FACTOR * worst


@functools.lru_cache(maxsize=None)
def case(sensor) -> Case:
    return Case(sensor)


def bins(p, R, interval, M, dtype=F64):
    """(bin, in range): floor((p + R) / interval) + 1, in range iff it lies in [0, M)"""
    b = np.floor((p.astype(dtype) + dtype(R)) / dtype(interval)).astype(np.int64) + 1
    return b, (b >= 0) & (b < M)


def round_half_away(v) -> np.ndarray:
    return np.where(v >= 0, np.floor(v + 0.5), -np.floor(-v + 0.5)).astype(np.int64)


def main_images(q, height_res, interval, dtype=F64):
    """The 24-layer occupancy image and the uint8 max-height image of points q (n, 3) in the map's frame: image[layer][x][y] =
    255 for layer = round(z / height_res + 2) in [0, 24); image[x][y] = max trunc((z + 2) * 4) clamped to 0 .. 255."""
    q = np.asarray(q).astype(dtype)
    M = int(2 * R_MAIN / interval)
    multi, single = np.zeros((N_LAYERS, M, M), np.uint8), np.zeros((M, M), np.uint8)
    bx, okx = bins(q[:, 0], R_MAIN, interval, M, dtype)
    by, oky = bins(q[:, 1], R_MAIN, interval, M, dtype)
    ok = okx & oky
    bx, by, z = bx[ok], by[ok], q[ok, 2]
    layer = round_half_away(z / dtype(height_res) + dtype(LIDAR_TO_GROUND))
    lok = (layer >= 0) & (layer < N_LAYERS)
    multi[layer[lok], bx[lok], by[lok]] = 255
    h = np.clip(np.trunc((z + dtype(LIDAR_TO_GROUND)) * dtype(4)), 0, 255).astype(np.uint8)
    np.maximum.at(single, (bx, by), h)
    return multi, single


def float_grid(q, interval, dtype=F64) -> np.ndarray:
    """The float max-height grid: R = 100, M = int(200 / interval + 1); a cell holds the largest z + 2 if positive, else 0"""
    q = np.asarray(q).astype(dtype)
    M = int(200.0 / interval + 1)
    grid = np.zeros((M, M), dtype)
    bx, okx = bins(q[:, 0], R_FLOAT, interval, M, dtype)
    by, oky = bins(q[:, 1], R_FLOAT, interval, M, dtype)
    h = q[:, 2] + dtype(LIDAR_TO_GROUND)
    ok = okx & oky & (h > 0)
    np.maximum.at(grid, (bx[ok], by[ok]), h[ok])
    return grid


def occupied(c: Case, name, keep_dropped=False) -> np.ndarray:
    """(M, M) bool: the cells of the 224-bin image that hold a point of the map with a non-zero label"""
    q = c.points(name, keep_dropped=keep_dropped)
    bx, okx = bins(q[:, 0], R_MAIN, c.interval, c.M)
    by, oky = bins(q[:, 1], R_MAIN, c.interval, c.M)
    out = np.zeros((c.M, c.M), bool)
    out[bx[okx & oky], by[okx & oky]] = True
    return out


def off_image_share(c: Case, name):
    """(share of the map's points off the 224-bin image, off on the low side of x, off on the high side of x)"""
    q = c.points(name)
    bx, okx = bins(q[:, 0], R_MAIN, c.interval, c.M)
    by, oky = bins(q[:, 1], R_MAIN, c.interval, c.M)
    return float(1.0 - (okx & oky).mean()), int((bx < 0).sum()), int((bx >= c.M).sum())


def compare_float(got, want, tol, what):
    """the float grid `got` against the reference `want`: the same occupied cells, every value within tol; returns the
    largest difference"""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff_occ = int(np.count_nonzero((got > 0) != (want > 0)))
    assert diff_occ == 0, f"{what}: {diff_occ} cells occupied in one grid only"
    d = float(np.abs(got - want).max())
    assert d <= tol, f"{what}: {d:.3e} from the float64 world, tol {tol:.3e}"
    return d


def compare_bytes(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    n = int(np.count_nonzero(got != want))
    assert n == 0, f"{what}: {n} bytes differ from the float64 world"
