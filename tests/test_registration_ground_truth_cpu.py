"""CPU: the registration stages against ground truth and a plain float64 ICP.  The other registration tests
compare the device byte for byte with checkers written from the same reading of the same contract; here the reference is
plain mathematics (ref64_registration.py) on a world whose true motions are known (ground_truth_cases.py), and the tolerance
comes from the reference alone: 8 times the distance between the same plain code in float32 and in float64, refused above
1e-4.

  a. conditions on the inputs, from the reference alone: the separation of the world's points, the sizes, the mixing of the
     entries, every tolerance within the cap, convergence to T_true, true correspondences, no near tie, the theta + 180 guess;
  b. the tests can fail: mutants of the reference's own target construction move its result by 100 tolerances or more;
  c. the checker compositions (submap_coarse_cases, submap_reg_cases, submap_vox_cases) against the reference and the truth.

What c measured (distance from the reference's iterate, largest over the matches; tol 2.6e-6 .. 1.3e-5):
  coarse, k = 1, 2, 3, 8:  3.4e-7  6.1e-7  7.2e-7  6.1e-7        fine D 1:  5.4e-7  6.3e-7  4.3e-7  2.1e-6
  whole D 4:               3.0e-7  4.7e-7  6.1e-7  2.0e-6        at map_leaf 0.2 up to 2.3e-6; from T_true at most 8.5e-7
"""
import numpy as np
import pytest

import fineicp_lib as fl
import ground_truth_cases as gt
import icp_lib
import ref64_registration as ref
import submap_coarse_cases as cc
import submap_reg_cases as sc
import submap_vox_cases as vc

N_MATCHES = 6
THREADS = 8


@pytest.fixture(scope="module")
def S():
    return gt.precompute()


# ---- a. conditions on the inputs ------------------------------------------------------------------------------------------------------
def test_the_world_keeps_its_points_apart_and_the_frames_their_sizes(S):
    xyz, nrm = gt.world()
    sep = gt.min_separation(xyz)
    print(f"{len(xyz)} world points, smallest distance {sep:.4f} m; frames of {[len(i) for i in S['ids']]} points")
    assert sep >= gt.SEPARATION > 0.2 * np.sqrt(3)
    assert 7000 <= len(xyz) <= 8000 and np.allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-15)
    assert all(2100 <= len(i) <= 2450 for i in S["ids"])
    assert len(S["matches"]) == N_MATCHES and 6 <= N_MATCHES <= 8
    assert [m[1] for m in S["maps"]] == [[0, 1, 2, 3, 4], [6, 5, 4, 3, 2], [3]]
    for f in range(1, gt.N_POSES):                                     # the path: about 4 m and ten degrees a step
        step = gt.inverse(S["poses"][f - 1]) @ S["poses"][f]
        assert 3.0 < np.linalg.norm(step[:3, 3]) < 5.0 and 7.0 < np.degrees(np.arctan2(step[1, 0], step[0, 0])) < 13.0


def test_the_maps_cross_a_sort_tile_and_mix_their_entries(S):
    for g, (origin, frames) in enumerate(S["maps"][:2]):
        concat = sum(len(S["ids"][f]) for f in frames)
        distinct = len(gt.ref_target(S, g)[0])
        print(f"map {g}: {concat} points in the concatenation, {distinct} distinct")
        assert concat > 2 * 4096 and 3000 <= distinct <= 4200
    for k, (q, g, _) in enumerate(S["matches"]):
        ids = gt.ref_target(S, g)[0]
        assert np.isin(S["ids"][q], ids).all(), f"match {k}: a query point no entry sees"
        T = S["truth"][k]
        assert np.linalg.norm(T[:3, 3]) < 1.0 and np.degrees(np.arccos((np.trace(T[:3, :3]) - 1) / 2)) < 3.0
        shares = [float(np.isin(S["ids"][q], S["ids"][f]).mean()) for f in S["maps"][g][1]]
        print(f"match {k}: the entries hold {np.round(shares, 3).tolist()} of the query's points")
        if len(shares) > 1:
            assert max(shares) < 1.0 and sum(s > 0.5 for s in shares) >= 3


@pytest.mark.parametrize("k", range(N_MATCHES))
def test_the_reference_converges_to_the_truth_without_a_near_tie(S, k):
    q, g, theta = S["matches"][k]
    ids, tx, _ = gt.ref_target(S, g)
    for setting in gt.SETTINGS:
        it, trace = gt.trajectory(k, setting)
        tol = gt.tol(k, setting)
        d8 = gt.dist(it[7], S["truth"][k])
        # on the construction itself (float64 points, zero residual) one more step lands on T_true; the fine setting starts that
        # step from the reference's coarse result, as the tool does (its made-up float32 start is no exact rotation, and an ICP
        # keeps what its start is off by: 2.5e-8 here)
        exact = gt.dist(gt.exact_step(k, setting, T=gt.trajectory(k, "coarse")[0][7] if setting == "fine" else None), S["truth"][k])
        _, idx, _, keep = trace[7]
        true_share = float((ids[idx[keep]] == S["ids"][q][keep]).mean())
        margin, ties = gt.near_ties(k, setting)
        print(f"match {k} {setting}: tol {tol:.2e}, iterate 8 from T_true {d8:.1e} (exact points: {exact:.1e}), true pairs "
              f"{true_share:.4f} of {int(keep.sum())}, smallest margin {margin:.2e} m")
        assert tol <= gt.CAP
        # the frames are rounded to float32 last: half an ulp of 32 m, 9.5e-7 m, in each coordinate of 2,300 pairs; their least
        # squares moves by that over sqrt(n), 2e-8, and a float32 start adds its own rounding, 6e-8
        assert exact <= 1e-9 and d8 <= 1e-7
        assert true_share >= 0.99 and keep.mean() >= 0.99
        assert margin > gt.GAP and not ties


def test_the_guess_turned_by_180_degrees_fits_ten_times_worse(S):
    for k, (q, g, theta) in enumerate(S["matches"]):
        _, tx, tn = gt.ref_target(S, g)
        good = ref.fitness(S["xyz32"][q], tx, gt.trajectory(k, "coarse")[0][7])
        back = ref.point_to_plane(S["xyz32"][q], tx, tn, ref.yaw_guess(theta, 1), gt.COARSE_D, 8)[-1]
        bad = ref.fitness(S["xyz32"][q], tx, back)
        print(f"match {k}: fitness {good:.3e} from theta, {bad:.3e} from theta + 180")
        assert bad >= 10 * good


# ---- b. mutants of the reference ------------------------------------------------------------------------------------------------------
def _mutants(S, g):
    n = len(S["maps"][g][1])
    mats = [gt.entry_matrix(S, g, e) for e in range(n)]
    keep = lambda R, t: (R, t, R, np.zeros(3))
    return {
        "one entry's matrix ignored": lambda e, R, t: keep(np.eye(3), np.zeros(3)) if e == 1 else keep(R, t),
        "every rotation transposed": lambda e, R, t: keep(R.T, t),
        "entry e under entry e + 1's matrix": lambda e, R, t: keep(mats[(e + 1) % n][:3, :3], mats[(e + 1) % n][:3, 3]),
        "the origin's entry dropped": lambda e, R, t: None if e == 2 else keep(R, t),
    }, {
        "coarse target normals left unrotated": lambda e, R, t: (R, t, np.eye(3), np.zeros(3)),
        "the translation added to the normals": lambda e, R, t: (R, t, R, t),
    }


@pytest.mark.parametrize("k", [0, 2])      # a match against map A and one against map B
def test_mutants_of_the_target_construction_move_the_reference(S, k):
    q, g, theta = S["matches"][k]
    src = S["xyz32"][q]
    at8, at1 = _mutants(S, g)
    moved = {}
    for name, mut in at8.items():                                    # judged at k = 8
        # under the fine setting (D 1), but the dropped entry under the whole setting (D 4): the query's points that only the
        # origin's entry sees lie at its rim, and with D 1 a part of them finds no partner at all and pulls nothing.  (A
        # dropped entry other than the origin's takes nothing from what these queries see; the GPU test's comparison of the
        # thinned cloud with the distinct visible world points is what catches that one.)
        setting, D = ("whole", gt.WHOLE_D) if "dropped" in name else ("fine", gt.FINE_D)
        _, tx, _ = gt.ref_target(S, g, mut)
        T = ref.point_to_point(src, tx, gt.start(S, k, setting), D, 8)[-1]
        moved[name] = gt.dist(T, gt.trajectory(k, setting)[0][7]) / gt.tol(k, setting)
    for name, mut in at1.items():                                    # the normals: judged at k = 1, where a wrong normal shows
        _, tx, tn = gt.ref_target(S, g, mut)
        T = ref.point_to_plane(src, tx, tn, gt.start(S, k, "coarse"), gt.COARSE_D, 1)[-1]
        moved[name] = gt.dist(T, gt.trajectory(k, "coarse")[0][0]) / gt.tol(k, "coarse")
    for setting in gt.SETTINGS:
        good = gt.trajectory(k, setting)[0]
        moved[f"the result returned inverted ({setting})"] = gt.dist(gt.inverse(good[7]), good[7]) / gt.tol(k, setting)
        # The transposed start is judged at k = 1: this world's relative yaws are a few degrees (the queries lie within 3
        # degrees of their map's origin), so by k = 8 the reference reaches T_true from the guess and from its transpose alike.
        # The comparisons at k = 1 are what catches a transposed guess.
        _, tx, tn = gt.ref_target(S, g)
        D = dict(coarse=gt.COARSE_D, fine=gt.FINE_D, whole=gt.WHOLE_D)[setting]
        G = gt.start(S, k, setting)
        Gt = np.eye(4)
        Gt[:3, :3], Gt[:3, 3] = G[:3, :3].T, G[:3, 3]
        T = (ref.point_to_plane(src, tx, tn, Gt, D, 1) if setting == "coarse" else ref.point_to_point(src, tx, Gt, D, 1))[-1]
        moved[f"the start transposed ({setting}, k = 1)"] = gt.dist(T, good[0]) / gt.tol(k, setting)
    for name, x in moved.items():
        print(f"match {k}: {name}: {x:.0f} tol")
    weak = {name: x for name, x in moved.items() if not x >= 100}
    assert not weak, weak


# ---- c. the checker compositions against the reference --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checkers():
    icp_lib.build()
    fl.build()


def test_the_coarse_checker_equals_the_reference_and_the_truth(S, checkers):
    maps, m = gt.checker_maps(S), gt.match_array(S)
    for k in gt.K:
        res, _ = cc.expected(S["rows"], maps, m, gt.fixed_params(gt.COARSE_D, k), None, threads=THREADS)
        for j in range(len(m)):
            want = gt.compared_iterate(f"coarse, match {j}, k = {k}", res[j, 0], j, "coarse", k)
            d = gt.dist(res[j, 0]["T"], want)
            print(f"coarse, match {j}, k = {k}: {d:.1e} from the reference, tol {gt.tol(j, 'coarse'):.1e}")
            assert d <= gt.tol(j, "coarse")
    res, best = cc.expected(S["rows"], maps, m, None, None, threads=THREADS)
    for j in range(len(m)):
        d = gt.dist(res[j, 0]["T"], S["truth"][j])
        print(f"coarse defaults, match {j}: {d:.1e} from T_true, state {res[j, 0]['state']}, best {best[j]}")
        assert d <= gt.tol(j, "coarse") and res[j, 0]["converged"] == 1 and best[j] == 0


@pytest.mark.parametrize("map_leaf", [None, 0.0, 0.2])
def test_the_fine_checkers_equal_the_reference_and_the_truth(S, checkers, map_leaf):
    maps, m = gt.checker_maps(S), gt.match_array(S)
    run = (lambda prm, g: sc.expected(S["clouds"], maps, m, prm, g, threads=THREADS)) if map_leaf is None else \
          (lambda prm, g: vc.expected(S["clouds"], maps, m, prm, map_leaf, g, threads=THREADS))
    table = [gt.perturbed(S, j) for j in range(len(m))]
    for setting, D, guesses in (("fine", gt.FINE_D, table), ("whole", gt.WHOLE_D, None)):
        for k in gt.K:
            res = run(gt.fixed_params(D, k), guesses)
            for j in range(len(m)):
                want = gt.compared_iterate(f"{setting}, match {j}, k = {k}", res[j], j, setting, k)
                d = gt.dist(res[j]["T"], want)
                print(f"{setting}, map_leaf {map_leaf}, match {j}, k = {k}: {d:.1e} from the reference, tol {gt.tol(j, setting):.1e}")
                assert d <= gt.tol(j, setting)
    coarse, best = cc.expected(S["rows"], maps, m, None, None, threads=THREADS)
    from_coarse = [coarse[j, best[j]]["T"].reshape(4, 4).copy() for j in range(len(m))]
    for setting, prm, guesses in (("fine", fl.params(**fl.FINE), from_coarse), ("whole", fl.params(**fl.WHOLE), None)):
        res = run(prm, guesses)
        for j in range(len(m)):
            d = gt.dist(res[j]["T"], S["truth"][j])
            print(f"{setting} settings, map_leaf {map_leaf}, match {j}: {d:.1e} from T_true, state {res[j]['state']} after {res[j]['iterations']}")
            assert d <= gt.tol(j, setting) and res[j]["converged"] == 1
