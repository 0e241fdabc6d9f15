"""ctypes loader for tests/fineicp/libfine_icp_oracle.so — the sequential C checker of the fine stage of the registration
tools: VoxelGrid<PointXYZIRCT>, point-to-point ICP (Umeyama through Eigen's JacobiSVD), the report
maths.  Tests only."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from bev_amd import ICP_RESULT_DTYPE, POINT_DTYPE, IcpParams, as_points

DIR = Path(__file__).resolve().parent / "fineicp"
SO = DIR / "libfine_icp_oracle.so"
_lib = None

# the tools' fine settings (bev_icp_fine_defaults / bev_icp_whole_defaults), restated
FINE = dict(max_correspondence_distance=1.0, transformation_epsilon=1e-6, euclidean_fitness_epsilon=0.01,
            max_iterations=100)
WHOLE = dict(max_correspondence_distance=4.0, transformation_epsilon=1e-6, euclidean_fitness_epsilon=0.001,
             max_iterations=200)


def params(**kw) -> IcpParams:
    d = dict(FINE)
    d.update(kw)
    return IcpParams(d["max_correspondence_distance"], d["transformation_epsilon"], d["euclidean_fitness_epsilon"],
                     d["max_iterations"], 0)


def build() -> None:
    r = subprocess.run(["make", "-C", str(DIR)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"make -C {DIR} failed:\n{r.stdout}")


def lib():
    global _lib
    if _lib is None:
        build()
        l = C.CDLL(str(SO))
        vp, u32 = C.c_void_p, C.c_uint32
        l.fine_voxel_irct.argtypes = [vp, u32, C.c_float, vp]
        l.fine_voxel_irct.restype = u32
        l.fine_nn.argtypes = [vp, u32, vp, u32, vp, vp]
        l.fine_svd3.argtypes = [vp, vp, vp, vp]
        l.fine_svd3.restype = C.c_int
        l.fine_rotation.argtypes = [vp, vp]
        l.fine_umeyama.argtypes = [vp, vp, u32, vp]
        l.fine_run.argtypes = [vp, u32, vp, u32, vp, C.POINTER(IcpParams), vp]
        l.fine_euler.argtypes = [vp, vp]
        l.fine_inverse3.argtypes = [vp, vp]
        l.fine_report.argtypes = [vp, vp, vp]
        l.icp_guess.argtypes = [C.c_float, C.c_int, vp]
        for f in ("fine_nn", "fine_rotation", "fine_umeyama", "fine_run", "fine_euler", "fine_inverse3", "fine_report",
                  "icp_guess"):
            getattr(l, f).restype = None
        _lib = l
    return _lib


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None and a.size else None


def voxel_irct(cloud, leaf=0.2):
    cloud = np.ascontiguousarray(cloud, dtype=POINT_DTYPE)
    out = np.zeros(max(len(cloud), 1), POINT_DTYPE)
    n = lib().fine_voxel_irct(_p(cloud), len(cloud), leaf, _p(out))
    return out[:n].copy()


def nn(tgt, queries):
    """Global nearest neighbour of every (x, y, z) query: (index uint32, squared distance float32)."""
    tgt = as_points(tgt)
    q = np.ascontiguousarray(np.asarray(queries, np.float32).reshape(-1, 3))
    idx = np.zeros(max(len(q), 1), np.uint32)
    dist = np.zeros(max(len(q), 1), np.float32)
    lib().fine_nn(_p(tgt), len(tgt), _p(q), len(q), _p(idx), _p(dist))
    return idx[: len(q)], dist[: len(q)]


def svd3(a):
    a = np.ascontiguousarray(a, np.float32).reshape(9)
    u, s, v = np.zeros(9, np.float32), np.zeros(3, np.float32), np.zeros(9, np.float32)
    sweeps = lib().fine_svd3(_p(a), _p(u), _p(s), _p(v))
    return u.reshape(3, 3), s, v.reshape(3, 3), sweeps


def rotation(sigma):
    sigma = np.ascontiguousarray(sigma, np.float32).reshape(9)
    r = np.zeros(9, np.float32)
    lib().fine_rotation(_p(sigma), _p(r))
    return r.reshape(3, 3)


def umeyama(src, dst):
    src = np.ascontiguousarray(src, np.float32).reshape(-1, 3)
    dst = np.ascontiguousarray(dst, np.float32).reshape(-1, 3)
    T = np.zeros(16, np.float32)
    lib().fine_umeyama(_p(src), _p(dst), len(src), _p(T))
    return T.reshape(4, 4)


def run(src, tgt, guess=None, prm: IcpParams | None = None):
    """One problem: an ICP_RESULT_DTYPE record."""
    src, tgt = as_points(src), as_points(tgt)
    g = np.ascontiguousarray((np.eye(4) if guess is None else np.asarray(guess)).astype(np.float32).reshape(16))
    prm = prm if prm is not None else params()
    out = np.zeros(1, ICP_RESULT_DTYPE)
    lib().fine_run(_p(src), len(src), _p(tgt), len(tgt), _p(g), C.byref(prm), _p(out))
    return out[0]


def tool_guess(angle_deg: float):
    T = np.zeros(16, np.float32)
    lib().icp_guess(angle_deg, 0, _p(T))
    return T.reshape(4, 4)


def euler(R):
    R = np.ascontiguousarray(R, np.float32).reshape(9)
    out = np.zeros(3, np.float32)
    lib().fine_euler(_p(R), _p(out))
    return out


def inverse3(m):
    m = np.ascontiguousarray(m, np.float32).reshape(9)
    out = np.zeros(9, np.float32)
    lib().fine_inverse3(_p(m), _p(out))
    return out.reshape(3, 3)


def report(T_fine, T_coarse):
    """(diff_xy, diff_yaw) of the top-part tool (float32)."""
    a = np.ascontiguousarray(T_fine, np.float32).reshape(16)
    b = np.ascontiguousarray(T_coarse, np.float32).reshape(16)
    out = np.zeros(2, np.float32)
    lib().fine_report(_p(a), _p(b), _p(out))
    return out[0], out[1]


def report_line(T_fine, T_coarse) -> str:
    """The report line as the tool's default ostream formatting writes it (%g of the float as double)."""
    xy, yaw = report(T_fine, T_coarse)
    return "%g %g\n" % (float(xy), float(yaw))


def fine(clouds, matches, guesses=None, prm: IcpParams | None = None, leaf=0.2, threads: int = 16):
    """The fine stage of a match list: the voxel grid of every frame named, then one ICP per match from guesses[m] (None:
    the yaw guess of angle_guess).  Returns (n,) ICP_RESULT_DTYPE; problems on up to `threads` threads."""
    from concurrent.futures import ThreadPoolExecutor

    names = sorted({int(q) for q, _, _ in matches} | {int(t) for _, t, _ in matches})
    with ThreadPoolExecutor(max(1, threads)) as ex:
        vox = dict(zip(names, ex.map(lambda f: voxel_irct(clouds[f], leaf), names)))
    res = np.zeros(len(matches), ICP_RESULT_DTYPE)

    def one(m):
        q, t, a = matches[m]
        g = tool_guess(float(a)) if guesses is None else guesses[m]
        res[m] = run(vox[int(q)], vox[int(t)], g, prm)

    with ThreadPoolExecutor(max(1, threads)) as ex:
        list(ex.map(one, range(len(matches))))
    return res
