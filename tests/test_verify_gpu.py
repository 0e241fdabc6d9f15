"""GPU: verification of registered matches (bev_verify.h, bev_capi_verify.hip) byte for byte against the
sequential checker tests/verify/verify_oracle.c: bev_verify_clouds over sizes, degenerate grids, thresholds and non-finite input;
the pair call on ragged packed frames, past one launch group, under another slice, in halves, behind the fine call without a
synchronise and on d_ordered; the host-buffer form; the submap call on maps of one to five entries, plain and thinned.  Every
output lies between guards."""
import numpy as np
import pytest

import bev_amd
import fineicp_lib as fl
import reg_cases as rc
import submap_reg_cases as sc
import submap_vox_cases as svc
import verify_lib as vl
from bev_amd import ICP_RESULT_DTYPE, MATCH_DTYPE, POINT_DTYPE, VERIFY_RESULT_DTYPE, BevError, synth, verify_params

pytestmark = pytest.mark.gpu
F32 = np.float32
R, V = ICP_RESULT_DTYPE.itemsize, VERIFY_RESULT_DTYPE.itemsize
GUARD, PATTERN = 4 * V, 0xA5
TH = (0.1, 0.3, 1.0, 3.0)


@pytest.fixture(scope="module", autouse=True)
def _checker():
    fl.build()
    vl.build()


@pytest.fixture(scope="module")
def ctx():
    c = bev_amd.BevContext(bev_amd.params_for_sensor("HDL_32E"), device=0, max_batch=4, max_points=25000)
    yield c
    c.close()


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(torch.device("cuda:0"))


def _results(Ts) -> np.ndarray:
    """ICP_RESULT_DTYPE records that carry the transforms and, everywhere else, bytes nobody may read into a count"""
    res = np.zeros(len(Ts), ICP_RESULT_DTYPE)
    res["fitness"], res["converged"], res["iterations"], res["state"] = 123.5, -3, 77, 9
    for k, T in enumerate(Ts):
        res["T"][k] = np.asarray(T, F32).reshape(16)
    return res


def _out(n):
    import torch

    return torch.full((n * V + GUARD,), PATTERN, dtype=torch.uint8, device=torch.device("cuda:0"))


def _read(d_out, n) -> np.ndarray:
    raw = d_out.cpu().numpy()
    assert np.all(raw[n * V:] == PATTERN), "the call wrote past its records"
    return raw[: n * V].view(VERIFY_RESULT_DTYPE).copy()


def _cloud(n, seed, box=10.0):
    rng = np.random.default_rng([int(seed), 0xC10D])
    return vl.points(np.c_[rng.uniform(-box, box, (n, 2)), rng.uniform(0.0, 2.0, n)])


def _check_clouds(ctx, src, tgt, T, prm, what):
    got = ctx.verify_clouds(src, tgt, T, prm)
    exp = vl.oracle(src, tgt, T, prm)
    assert got.tobytes() == exp.tobytes(), f"{what}: {got} != {exp}"
    return got


# ---- bev_verify_clouds ------------------------------------------------------------------------------------------------------
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1025, 5000]
MIXED = [(0, 5000), (5000, 0), (1, 257), (257, 1), (63, 1025), (1025, 63), (64, 65), (65, 64), (255, 5000), (5000, 255),
         (256, 1025), (1025, 256)]


@pytest.mark.parametrize("ns,nt", [(n, n) for n in SIZES] + MIXED)
def test_verify_clouds_sizes_equal_the_checker(ctx, ns, nt):
    # the box shrinks with the size, so that nearest distances stay spread over the thresholds
    box = max(0.5, 0.25 * np.sqrt(max(ns, nt, 1)))
    T = rc.rigid(3.0, 0.2, -0.1)
    r = _check_clouds(ctx, _cloud(ns, 10 + ns, box), _cloud(nt, 20 + nt, box), T, verify_params(TH), (ns, nt))
    assert r["n_query"] == ns and r["n_target"] == nt
    if ns >= 255 and nt >= 255:
        assert 0 < r["query_within"][0] < r["query_within"][3] and 0 < r["target_within"][0] < r["target_within"][3]


def test_verify_clouds_degenerate_grids_and_thresholds(ctx):
    rng = np.random.default_rng(5)
    T = rc.rigid(-2.0, 0.1, 0.15)
    q = _cloud(3000, 31, 15.0)
    big = _cloud(20000, 32, 20.0)  # ceil(sqrt(n)) = 142 > 128: the grid's dimension at its cap
    r = _check_clouds(ctx, q, big, T, verify_params(TH), "20000 points")
    assert r["n_target"] == 20000 and r["query_within"][1] > 0
    _check_clouds(ctx, big, big, T, verify_params((0.05, 0.2)), "20000 against 20000")
    column = vl.points(np.c_[np.full(500, 1.25), np.full(500, -3.5), rng.uniform(0, 30, 500)])  # one (x, y): s = 0
    _check_clouds(ctx, _cloud(700, 33, 3.0), column, T, verify_params(TH), "one distinct (x, y)")
    _check_clouds(ctx, column, _cloud(700, 33, 3.0), T, verify_params(TH), "one distinct (x, y) as the query")
    line = vl.points(np.c_[np.linspace(-20, 20, 900), np.full(900, 2.0), np.zeros(900)])  # collinear: ny = 1
    _check_clouds(ctx, _cloud(800, 34, 20.0), line, T, verify_params(TH), "collinear")
    far = _cloud(600, 35, 5.0)
    far["x"] += F32(500.0)  # wholly outside the target's bounds: every cell coordinate clamps
    r = _check_clouds(ctx, far, _cloud(900, 36, 5.0), np.eye(4), verify_params(TH), "outside")
    assert not r["query_within"].any() and not r["target_within"].any()
    a, b = _cloud(4000, 37, 6.0), _cloud(3500, 38, 6.0)
    b[:500] = a[:500]
    r = _check_clouds(ctx, a, b, np.eye(4), verify_params((1e-3,)), "1e-3 alone")
    assert 500 <= r["query_within"][0] < 600
    r = _check_clouds(ctx, a, b, T, verify_params((1e-3, 1.0, 10.0, 1e3)), "up to 1e3")  # the early stop never fires
    assert r["query_within"][3] == 4000 and r["target_within"][3] == 3500
    r = _check_clouds(ctx, a, b, T, verify_params(tuple(0.02 * 2.0 ** k for k in range(8))), "eight thresholds")
    assert np.all(np.diff(r["query_within"].astype(np.int64)) >= 0)


def test_verify_clouds_boundary_and_non_finite(ctx):
    c = vl.lattice(200, 2, extent=400 * 32)
    T = vl.shift4(0.25)
    at = _check_clouds(ctx, c, c, T, verify_params((0.25,)), "at the boundary")
    below = _check_clouds(ctx, c, c, T, verify_params((float(np.nextafter(F32(0.25), F32(0))),)), "below it")
    assert at["query_within"][0] == at["target_within"][0] == 200
    assert below["query_within"][0] == below["target_within"][0] == 0
    same = _check_clouds(ctx, c, c, np.eye(4), verify_params(TH), "identical")
    assert same["query_within"][:4].tolist() == [200] * 4 == same["target_within"][:4].tolist()
    for bad in (np.nan, np.inf):
        Tb = np.eye(4, dtype=F32)
        Tb[2, 3] = bad
        r = _check_clouds(ctx, c, c, Tb, verify_params(TH), f"T with {bad}")
        assert r["n_query"] == 0 and r["n_target"] == 200 and not r["query_within"].any() and not r["target_within"].any()
    src, tgt = _cloud(1500, 41, 5.0), _cloud(1400, 42, 5.0)
    src["x"][::9], src["y"][1::13], src["z"][2::17] = np.nan, np.inf, -np.inf
    tgt["x"][::7], tgt["z"][3::11] = -np.inf, np.nan
    src["x"][4], tgt["y"][5] = F32(-0.0), F32(-0.0)
    r = _check_clouds(ctx, src, tgt, rc.rigid(1.0, 0.05, 0.0), verify_params(TH), "non-finite points")
    assert r["n_query"] < 1500 and r["n_target"] < 1400
    allnan = vl.points(np.full((70, 3), np.nan))
    for s, t in ((allnan, tgt), (src, allnan)):
        r = _check_clouds(ctx, s, t, np.eye(4), verify_params(TH), "one side without a searchable point")
        assert not r["query_within"].any() and not r["target_within"].any()


BAD_THRESHOLDS = [(), (0.0,), (-1.0,), (np.nan,), (np.inf,), (0.2, 0.2), (0.3, 0.2), (0.1, 0.2, 0.0, 0.4), tuple(range(1, 10))]


def _bad_params():
    out = [verify_params(t) for t in BAD_THRESHOLDS]
    tail = verify_params((0.1, 0.2))
    tail.threshold[5] = 0.5  # an unused slot that is not 0
    return out + [tail]


def test_refusals(ctx):
    import torch

    c = _cloud(100, 50)
    for prm in _bad_params():
        with pytest.raises(BevError):
            ctx.verify_clouds(c, c, np.eye(4), prm)
    clouds = [c, c]
    offs = np.array([0, 100, 200], np.uint64)
    d_clouds, d_res, d_out = _dev(rc.packed(clouds)), _dev(_results([np.eye(4)])), _out(1)
    torch.cuda.synchronize()
    m = np.array([(0, 1, 0.0)], MATCH_DTYPE)
    maps = sc.Maps()
    maps.add([(0, sc.IDENTITY)])

    def pair(matches=m, offsets=offs, prm=verify_params(TH)):
        ctx.verify_registration_device(2, d_clouds.data_ptr(), offsets, matches, d_res.data_ptr(), d_out.data_ptr(), prm)

    def submap(matches=np.array([(1, 0, 0.0)], MATCH_DTYPE), prm=verify_params(TH), map_leaf=0.0, arrays=maps.arrays()):
        ctx.submap_verify_registration_device(2, d_clouds.data_ptr(), offs, *arrays, matches, d_res.data_ptr(), d_out.data_ptr(),
                                              map_leaf, prm)

    bad_calls = [lambda p=p: pair(prm=p) for p in _bad_params()] + [lambda p=p: submap(prm=p) for p in _bad_params()]
    for leaf in (0.0, -0.2, np.nan, np.inf):
        bad_calls += [lambda l=leaf: pair(prm=verify_params(TH, leaf=l)), lambda l=leaf: submap(prm=verify_params(TH, leaf=l))]
    for q, t in ((-1, 0), (2, 0), (0, -1), (0, 2)):
        bad_calls.append(lambda q=q, t=t: pair(matches=np.array([(q, t, 0.0)], MATCH_DTYPE)))
    bad_calls.append(lambda: pair(offsets=np.array([0, 200, 100], np.uint64)))
    bad_calls += [lambda: submap(matches=np.array([(2, 0, 0.0)], MATCH_DTYPE)), lambda: submap(matches=np.array([(0, 1, 0.0)], MATCH_DTYPE)),
                  lambda: submap(map_leaf=-0.1), lambda: submap(map_leaf=np.nan)]
    bad_entry = sc.Maps()
    bad_entry.add([(5, sc.IDENTITY)])
    bad_calls.append(lambda: submap(arrays=bad_entry.arrays()))
    for call in bad_calls:
        with pytest.raises(BevError):
            call()
    for call in (lambda: ctx.verify_registration_batch(clouds, m, _results([np.eye(4)]), verify_params((0.3, 0.2))),
                 lambda: ctx.verify_registration_batch(clouds, [(0, 2, 0.0)], _results([np.eye(4)]), verify_params(TH))):
        with pytest.raises(BevError):
            call()
    ctx.synchronize()
    _read(d_out, 0)  # nothing was launched: not a byte of the output has changed
    pair()
    submap()
    ctx.synchronize()


# ---- the pair call ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pack():
    """the ragged pack, its voxel clouds from the checker and a match list with the transforms that go with it"""
    p = rc.ragged_pack()
    H = p.half
    vox = [fl.voxel_irct(c, 0.2) for c in p.clouds]
    rows, Ts = [], []
    base = sorted(set(range(0, H, 7)) | set(p.special.values()))
    base = [i for i in base if i not in (11, 12)]  # frames 11, 12 and their copies: named by no match
    for i in base:  # a frame onto its moved copy under the motion that made it
        rows.append((i, H + i, 0.0))
        Ts.append(rc.rigid(p.yaw[i], p.tr[i, 0], p.tr[i, 1]))
    for i in base[:12]:  # a frame against itself under the identity
        rows.append((i, i, 0.0))
        Ts.append(np.eye(4, dtype=F32))
    big = int(np.argmax([len(c) for c in p.clouds[:H]]))
    for i in base[:25]:  # one target named by many matches, under motions that fit badly
        rows.append((i, big, 0.0))
        Ts.append(rc.rigid(5.0 * (i % 5), 0.3, -0.2))
    nanT = np.eye(4, dtype=F32)
    nanT[0, 0] = np.nan
    rows.append((base[3], H + base[3], 0.0))
    Ts.append(nanT)
    m = np.array(rows, MATCH_DTYPE)
    return dict(pack=p, vox=vox, m=m, res=_results(Ts), d_clouds=_dev(rc.packed(p.clouds)))


def _expected_pairs(vox, m, res, prm):
    return np.array([vl.oracle(vox[int(q)], vox[int(t)], res["T"][k], prm) for k, (q, t, _) in enumerate(m)], VERIFY_RESULT_DTYPE)


def _pair_call(ctx, P, m, res, prm):
    import torch

    d_res, d_out = _dev(res) if len(res) else _dev(np.zeros(1, ICP_RESULT_DTYPE)), _out(len(m))
    torch.cuda.synchronize()
    ctx.verify_registration_device(len(P["pack"].clouds), P["d_clouds"].data_ptr(), P["pack"].offsets, m, d_res.data_ptr(),
                                   d_out.data_ptr(), prm)
    ctx.synchronize()
    return _read(d_out, len(m))


def test_pair_call_on_ragged_frames_equals_the_checker(ctx, pack, monkeypatch):
    prm = verify_params(TH)
    m, res = pack["m"], pack["res"]
    exp = _expected_pairs(pack["vox"], m, res, prm)
    got = _pair_call(ctx, pack, m, res, prm)
    assert got.tobytes() == exp.tobytes()
    # a frame onto its moved copy: the voxel grids of the two differ, yet most points find a neighbour within 0.3 m both ways
    n_copy = sum(1 for q, t, _ in m if t == q + pack["pack"].half) - 1
    ok = [k for k in range(n_copy) if exp["n_query"][k] > 200]
    assert len(ok) > 20 and all(exp["query_within"][k][1] > 0.8 * exp["n_query"][k] for k in ok)
    assert all(exp["target_within"][k][1] > 0.8 * exp["n_target"][k] for k in ok)
    self_rows = [k for k, (q, t, _) in enumerate(m) if q == t and exp["n_query"][k]]
    assert self_rows and all(exp["query_within"][k][0] == exp["n_query"][k] == exp["target_within"][k][0] for k in self_rows)
    assert exp["n_query"][-1] == 0 and not exp["query_within"][-1].any() and not exp["target_within"][-1].any()  # the NaN T
    # no match, one match
    assert len(_pair_call(ctx, pack, m[:0], res[:0], prm)) == 0
    assert _pair_call(ctx, pack, m[:1], res[:1], prm).tobytes() == exp[:1].tobytes()
    # one call against two calls over halves
    h = len(m) // 2
    halves = np.concatenate([_pair_call(ctx, pack, m[:h], res[:h], prm), _pair_call(ctx, pack, m[h:], res[h:], prm)])
    assert halves.tobytes() == exp.tobytes()
    # small clouds cut into several workgroups
    monkeypatch.setenv("BEV_VERIFY_SLICE", "64")
    assert _pair_call(ctx, pack, m, res, prm).tobytes() == exp.tobytes()
    monkeypatch.delenv("BEV_VERIFY_SLICE")
    # other thresholds and another leaf
    prm2 = verify_params((0.05, 0.5), leaf=0.35)
    vox2 = {f: fl.voxel_irct(pack["pack"].clouds[f], 0.35) for f in set(m["query_idx"][:20]) | set(m["match_idx"][:20])}
    assert _pair_call(ctx, pack, m[:20], res[:20], prm2).tobytes() == _expected_pairs(vox2, m[:20], res[:20], prm2).tobytes()
    # the host-buffer form
    assert ctx.verify_registration_batch(pack["pack"].clouds, m, res, prm).tobytes() == exp.tobytes()


def test_pair_call_past_one_launch_group(ctx, monkeypatch):
    small = [_cloud(n, 700 + n, 2.0) for n in (0, 1, 5, 40, 90, 130, 200, 257)]
    vox = [fl.voxel_irct(c, 0.2) for c in small]
    rng = np.random.default_rng(9)
    n = 1025
    m = np.array([(int(rng.integers(0, 8)), int(rng.integers(0, 8)), 0.0) for _ in range(n)], MATCH_DTYPE)
    res = _results([rc.rigid(rng.uniform(-3, 3), *rng.uniform(-0.2, 0.2, 2)) for _ in range(n)])
    prm = verify_params(TH)
    P = dict(pack=type("P", (), dict(clouds=small, offsets=np.r_[0, np.cumsum([len(c) for c in small])].astype(np.uint64)))(),
             d_clouds=_dev(rc.packed(small)))
    exp = _expected_pairs(vox, m, res, prm)
    assert _pair_call(ctx, P, m, res, prm).tobytes() == exp.tobytes()
    monkeypatch.setenv("BEV_VERIFY_SLICE", "64")
    assert _pair_call(ctx, P, m, res, prm).tobytes() == exp.tobytes()
    assert exp["query_within"][:, 3].max() > 100


def test_pair_call_behind_the_fine_call_without_a_synchronise(ctx, pack):
    import torch

    p, H = pack["pack"], pack["pack"].half
    rows = [(i, H + i, float(p.yaw[i])) for i in range(0, 60, 3) if i not in p.degenerate]
    m = np.array(rows, MATCH_DTYPE)
    d_res, d_out = torch.zeros(len(m) * R, dtype=torch.uint8, device="cuda:0"), _out(len(m))
    torch.cuda.synchronize()
    prm = verify_params(TH)
    ctx.fine_registration_device(len(p.clouds), pack["d_clouds"].data_ptr(), p.offsets, m, d_res.data_ptr(), params=fl.params(**fl.WHOLE))
    ctx.verify_registration_device(len(p.clouds), pack["d_clouds"].data_ptr(), p.offsets, m, d_res.data_ptr(), d_out.data_ptr(), prm)
    ctx.synchronize()
    res = d_res.cpu().numpy().view(ICP_RESULT_DTYPE)
    got = _read(d_out, len(m))
    assert got.tobytes() == _expected_pairs(pack["vox"], m, res, prm).tobytes()
    good = [k for k in range(len(m)) if res["converged"][k] and got["n_query"][k] > 300]
    assert len(good) > 5 and np.median([got["query_within"][k][1] / got["n_query"][k] for k in good]) > 0.7


def test_pair_call_on_d_ordered():
    import torch

    p = bev_amd.params_for_sensor("HDL_32E")
    S, F = p.slots, 4
    frames = [synth.sweep(p, 81000 + i, keep=0.97, n_dup=500) for i in range(F)]
    c = bev_amd.BevContext(p, device=0, max_batch=F, max_points=max(len(f) for f in frames))
    try:
        offs = np.r_[0, np.cumsum([len(f) for f in frames])].astype(np.uint64)
        d_in = _dev(np.concatenate(frames))
        d_ord = torch.zeros(F * S * 32, dtype=torch.uint8, device="cuda:0")
        d_multi = torch.zeros(F * p.n_layers * p.mat_size ** 2, dtype=torch.uint8, device="cuda:0")
        d_single = torch.zeros(F * p.mat_size ** 2, dtype=torch.uint8, device="cuda:0")
        m = np.array([(0, 1, 0.0), (2, 3, 0.0), (3, 3, 0.0)], MATCH_DTYPE)
        res = _results([rc.rigid(0.5, 0.1, 0.0), rc.rigid(-0.5, 0.0, 0.1), np.eye(4)])
        d_res, d_out = _dev(res), _out(len(m))
        torch.cuda.synchronize()
        prm = verify_params(TH)
        c.process_device(F, d_in.data_ptr(), offs, d_ord.data_ptr(), d_multi.data_ptr(), d_single.data_ptr())
        c.verify_registration_device(F, d_ord.data_ptr(), None, m, d_res.data_ptr(), d_out.data_ptr(), prm)  # no synchronise
        c.synchronize()
        ordered = d_ord.cpu().numpy().view(POINT_DTYPE).reshape(F, S)
        vox = [fl.voxel_irct(o, 0.2) for o in ordered]
        got = _read(d_out, len(m))
        assert got.tobytes() == _expected_pairs(vox, m, res, prm).tobytes()
        assert got["n_query"].min() > 1000 and got["query_within"][2][0] == got["n_query"][2]
    finally:
        c.close()


# ---- the submap call ------------------------------------------------------------------------------------------------------
def _general(seed):
    """a row-major 3 x 4 that is no rigid motion: a small shear and scale on top of a rotation"""
    rng = np.random.default_rng([int(seed), 0x6E])
    M = np.eye(4)
    M[:3, :3] = np.asarray(rc.rigid(rng.uniform(-20, 20), 0, 0), np.float64)[:3, :3] @ (np.eye(3) + rng.uniform(-0.03, 0.03, (3, 3)))
    M[:3, 3] = rng.uniform(-1, 1, 3)
    return M[:3].astype(F32).reshape(12)


@pytest.mark.parametrize("map_leaf", [0.0, 0.4])
def test_submap_call_equals_the_checker(ctx, map_leaf, monkeypatch):
    import torch

    clouds = [rc.scene(n, 900 + k) for k, n in enumerate((1500, 1200, 900, 1700, 1100, 1300, 800, 0))]
    maps = sc.Maps()
    g1 = maps.add([(0, _general(1))])
    g3 = maps.add([(1, _general(2)), (0, sc.IDENTITY), (2, _general(3))])  # frame 0 in two maps
    g5 = maps.add([(3, _general(4)), (4, _general(5)), (3, _general(6)), (5, _general(7)), (2, _general(8))])
    g0 = maps.add([])  # a map without entries
    gn = maps.add([(7, sc.IDENTITY)])  # a map whose only entry is an empty frame
    rows = [(6, g1, 0), (0, g1, 0), (6, g3, 0), (1, g3, 0), (6, g5, 0), (3, g5, 0), (2, g0, 0), (4, gn, 0), (7, g3, 0), (5, g5, 0)]
    m = sc.matches(rows)
    nanT = np.eye(4, dtype=F32)
    nanT[1, 1] = np.nan
    Ts = [rc.rigid(2.0 * k, 0.1 * k, -0.05 * k) for k in range(len(m) - 1)] + [nanT]
    Ts[1] = np.r_[_general(1), [0, 0, 0, 1]].astype(F32).reshape(4, 4)  # frame 0 under its own entry matrix: onto itself
    res = _results(Ts)
    prm = verify_params(TH)
    vox = svc.voxel_clouds(clouds, range(len(clouds)))
    tgt = {g: svc.thin(sc.target(vox, maps.entries(g)), map_leaf) for g in range(len(maps))}
    exp = np.array([vl.oracle(vox[int(q)], tgt[int(g)], res["T"][k], prm) for k, (q, g, _) in enumerate(m)], VERIFY_RESULT_DTYPE)
    offs = np.r_[0, np.cumsum([len(c) for c in clouds])].astype(np.uint64)
    d_clouds, d_res = _dev(rc.packed(clouds)), _dev(res)

    def call(mm=m, first=0):
        d_out = _out(len(mm))
        d_r = _dev(res[first:first + len(mm)])
        torch.cuda.synchronize()
        ctx.submap_verify_registration_device(len(clouds), d_clouds.data_ptr(), offs, *maps.arrays(), mm, d_r.data_ptr(),
                                              d_out.data_ptr(), map_leaf, prm)
        ctx.synchronize()
        return _read(d_out, len(mm))

    got = call()
    assert got.tobytes() == exp.tobytes(), (got, exp)
    if map_leaf == 0:
        assert exp["n_target"][1] == len(vox[0]) and exp["query_within"][1][1] == exp["n_query"][1]
        assert exp["n_target"][4] == sum(len(vox[f]) for f in (3, 4, 3, 5, 2))
    else:
        assert exp["n_target"][4] < sum(len(vox[f]) for f in (3, 4, 3, 5, 2))
    assert exp["n_target"][6] == 0 == exp["n_target"][7] and not exp["query_within"][6:8].any() and not exp["target_within"][6:8].any()
    assert exp["n_query"][8] == 0 and exp["n_query"][9] == 0
    monkeypatch.setenv("BEV_VERIFY_SLICE", "64")
    assert call().tobytes() == exp.tobytes()
    monkeypatch.setenv("BEV_SUBMAP_REG_GROUP", "1")  # every map a launch group of its own (read when a context is made)
    c2 = bev_amd.BevContext(bev_amd.params_for_sensor("HDL_32E"), device=0, max_batch=2, max_points=5000)
    try:
        d_out = _out(len(m))
        torch.cuda.synchronize()
        c2.submap_verify_registration_device(len(clouds), d_clouds.data_ptr(), offs, *maps.arrays(), m, d_res.data_ptr(),
                                             d_out.data_ptr(), map_leaf, prm)
        c2.synchronize()
        assert _read(d_out, len(m)).tobytes() == exp.tobytes()
    finally:
        c2.close()
    assert np.concatenate([call(m[:4]), call(m[4:], 4)]).tobytes() == exp.tobytes()


def test_submap_call_on_the_mirror_tie(ctx):
    import torch

    clouds, maps, m = sc.mirror_tie()
    vox = svc.voxel_clouds(clouds, range(len(clouds)))
    res = _results([np.eye(4), vl.shift4(0.5)])
    prm = verify_params((0.25, 0.5, 0.6))  # the tie's distance is sqrt(0.25 + 1 / 64) = 0.5154
    exp = np.array([vl.oracle(vox[int(q)], sc.target(vox, maps.entries(int(g))), res["T"][k], prm) for k, (q, g, _) in enumerate(m)],
                   VERIFY_RESULT_DTYPE)
    offs = np.r_[0, np.cumsum([len(c) for c in clouds])].astype(np.uint64)
    d_clouds, d_res, d_out = _dev(rc.packed(clouds)), _dev(res), _out(len(m))
    torch.cuda.synchronize()
    ctx.submap_verify_registration_device(len(clouds), d_clouds.data_ptr(), offs, *maps.arrays(), m, d_res.data_ptr(), d_out.data_ptr(),
                                          0.0, prm)
    ctx.synchronize()
    got = _read(d_out, len(m))
    assert got.tobytes() == exp.tobytes()
    # every source point is equally far from its image in either entry: both images count, whatever the entries' order
    assert got["n_query"].tolist() == [400, 400] and got["n_target"].tolist() == [800, 800]
    assert got["query_within"][0][:3].tolist() == [0, 0, 400] and got["target_within"][0][:3].tolist() == [0, 0, 800]
    assert got["query_within"][1][:3].tolist() == [400, 400, 400] and got["target_within"][1][:3].tolist() == [400, 400, 400]
