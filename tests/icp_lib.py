"""ctypes loader for tests/icp/libicp_oracle.so — the sequential C checker of the coarse point-to-plane ICP
(DESIGN.md §6c).  Tests only."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from bev_amd import ICP_RESULT_DTYPE, IcpParams, icp_params

DIR = Path(__file__).resolve().parent / "icp"
SO = DIR / "libicp_oracle.so"
_lib = None


def build() -> None:
    r = subprocess.run(["make", "-C", str(DIR)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"make -C {DIR} failed:\n{r.stdout}")


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(str(SO))
        vp, u32, d = C.c_void_p, C.c_uint32, C.c_double
        l.icp_sin.argtypes = l.icp_cos.argtypes = [d]
        l.icp_sin.restype = l.icp_cos.restype = d
        l.icp_nn.argtypes = [vp, u32, vp, u32, vp, vp]
        l.icp_nn.restype = None
        l.icp_solve.argtypes = [vp, vp, vp]
        l.icp_solve.restype = None
        l.icp_increment.argtypes = [vp, vp]
        l.icp_increment.restype = None
        l.icp_guess.argtypes = [C.c_float, C.c_int, vp]
        l.icp_guess.restype = None
        l.icp_run.argtypes = [vp, u32, vp, u32, vp, C.POINTER(IcpParams), vp]
        l.icp_run.restype = None
        l.icp_best.argtypes = [d, d]
        l.icp_best.restype = C.c_int
        _lib = l
    return _lib


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _pn12(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1, 12))


def sin(x: float) -> float:
    return lib().icp_sin(x)


def cos(x: float) -> float:
    return lib().icp_cos(x)


def nn(tgt, queries):
    """Global nearest neighbour of every query row (12-float records): (index uint32, squared distance float32);
    index 0xffffffff when the target has no searchable point."""
    tgt, q = _pn12(tgt), _pn12(queries)
    idx = np.zeros(max(len(q), 1), np.uint32)
    dist = np.zeros(max(len(q), 1), np.float32)
    lib().icp_nn(_p(tgt), len(tgt), _p(q), len(q), _p(idx), _p(dist))
    return idx[: len(q)], dist[: len(q)]


def solve(ata, atb):
    ata = np.ascontiguousarray(ata, np.float64).reshape(36)
    atb = np.ascontiguousarray(atb, np.float64).reshape(6)
    x = np.zeros(6, np.float64)
    lib().icp_solve(_p(ata), _p(atb), _p(x))
    return x


def increment(x):
    x = np.ascontiguousarray(x, np.float64).reshape(6)
    T = np.zeros(16, np.float32)
    lib().icp_increment(_p(x), _p(T))
    return T.reshape(4, 4)


def tool_guess(angle_deg: float, which: int):
    T = np.zeros(16, np.float32)
    lib().icp_guess(angle_deg, which, _p(T))
    return T.reshape(4, 4)


def run(src, tgt, guess=None, params: IcpParams | None = None):
    """One problem: an ICP_RESULT_DTYPE record."""
    src, tgt = _pn12(src), _pn12(tgt)
    g = np.eye(4, dtype=np.float32) if guess is None else np.asarray(guess, np.float32)
    g = np.ascontiguousarray(g.reshape(16))
    prm = params if params is not None else icp_params()
    out = np.zeros(1, ICP_RESULT_DTYPE)
    lib().icp_run(_p(src) if len(src) else None, len(src), _p(tgt) if len(tgt) else None, len(tgt), _p(g),
                  C.byref(prm), _p(out))
    return out[0]


def best(f0: float, f1: float) -> int:
    return lib().icp_best(f0, f1)


def coarse(pn_clouds, matches, params: IcpParams | None = None, threads: int = 16):
    """The tool's coarse loop: (results (n, 2) ICP_RESULT_DTYPE, best (n,) int32), the problems on up to `threads`
    threads (ctypes releases the GIL)."""
    from concurrent.futures import ThreadPoolExecutor

    clouds = [_pn12(c_) for c_ in pn_clouds]
    n = len(matches)
    res = np.zeros((n, 2), ICP_RESULT_DTYPE)

    def one(k):
        m, g = divmod(k, 2)
        q, t, a = matches[m]
        res[m, g] = run(clouds[int(q)], clouds[int(t)], tool_guess(float(a), g), params)

    with ThreadPoolExecutor(max(1, threads)) as ex:
        list(ex.map(one, range(2 * n)))
    bst = np.array([best(float(r[0]["fitness"]), float(r[1]["fitness"])) for r in res], np.int32)
    return res, bst
