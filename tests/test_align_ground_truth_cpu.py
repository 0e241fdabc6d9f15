"""CPU: the conditions on the inputs of the ground-truth test of the translation guess (tests/align_cases.py), on
the sequential checker alone: its winning translation is within one cell per axis of the truth for every query and best picks
the true flip; the tolerance the device's hand-over is held to is below the cap; and the stage is needed — the same float64 ICP
from the bare yaw guess misses the truth by more than half a metre for at least half of the queries."""
import numpy as np

import align_cases as ac
import ground_truth_cases as gt


def test_the_checker_is_within_one_cell_and_picks_the_true_flip():
    """the bound comes from the grid: half a cell of quantisation on either side, plus the yaw left after the search over k
    (at most 1 degree of the 3 between a turn and its sector) at the walls' range"""
    S = ac.case()
    _, res, best, det = ac.checker_table()
    assert np.array_equal(best, S["flip"])
    assert (S["flip"] == 0).sum() >= 20 and (S["flip"] == 1).sum() >= 20
    r = np.linalg.norm(S["shift"], axis=1)
    assert ac.MIN_SHIFT <= r.min() and r.max() <= ac.MAX_SHIFT
    worst = 0.0
    for k in range(len(S["hits"])):
        T = res[k, S["flip"][k]]["T"]
        e = np.abs(np.array([T[3], T[7]], np.float64) - S["shift"][k])
        worst = max(worst, float(e.max()))
        assert (e <= ac.CELL).all(), (k, e)
        assert res[k, S["flip"][k]]["converged"] == 1 and abs(int(det[k, S["flip"][k]]["k"])) <= ac.YAW_STEPS
    print("worst error of the checker's translation per axis:", worst, "m of a cell of", ac.CELL)
    assert worst <= ac.CELL


def test_the_stage_is_needed_and_the_hand_over_tolerance_is_below_the_cap():
    S = ac.case()
    n = len(S["hits"])
    ac.precompute([(k, "float64", True) for k in range(n)] + [(k, d) for k in ac.HAND_OVER for d in ("float64", "float32")])
    miss = np.array([np.linalg.norm(ac.trajectory(k, "float64", True)[-1][:2, 3] - S["shift"][k]) for k in range(n)])
    print("the float64 ICP from the bare yaw guess misses the truth by more than 0.5 m for", int((miss > 0.5).sum()), "of", n,
          "queries; smallest miss", float(miss.min()))
    assert (miss > 0.5).sum() * 2 >= n
    for k in ac.HAND_OVER:  # from the table the same ICP comes home, and float32 against float64 stays under the cap
        t = ac.tol(k)
        err = gt.dist(ac.trajectory(k)[-1], S["T_true"][k])
        print("hit", k, "tolerance", t, "distance of the reference's iterate 8 from the truth", err)
        assert t <= gt.CAP
        assert np.linalg.norm(ac.trajectory(k)[-1][:2, 3] - S["shift"][k]) < 0.5 * 0.5
