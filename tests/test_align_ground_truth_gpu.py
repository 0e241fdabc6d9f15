"""GPU: the translation guess of retrieved pairs against ground truth (tests/align_cases.py): on the world of
ground_truth_cases.py, for 49 queries displaced by 1.5 ... 3 m from their database frames, the device's table equals the
checker's, its winning translation is within one cell per axis of P_db^-1 P_q, best picks the true flip, and the table handed as
it is to bev_fine_registration_device_resident under the top-part fine settings (D = 1) gives the iterates of a plain float64
ICP from the same start, within §6o's tolerance (8 times float32 against float64 of that plain code, refused above 1e-4).
test_align_ground_truth_cpu.py asserts the conditions on the inputs."""
import numpy as np
import pytest
import torch

import align_cases as ac
import bev_amd
import ground_truth_cases as gt
from align_gpu_lib import D, R, guarded, guard_ok
from bev_amd import ALIGN_DETAIL_DTYPE, ICP_RESULT_DTYPE
from packed_cases import _dev, _p, _pack

pytestmark = pytest.mark.gpu


def test_translation_flip_and_hand_over():
    S, prm = ac.case(), ac.params()
    frames, hits = ac.frames(S), S["hits"]
    n_db, n = len(S["db_clouds"]), len(hits)
    ac.precompute([(k, d) for k in ac.HAND_OVER for d in ("float64", "float32")])
    want_grids, want_res, want_best, want_det = ac.checker_table()
    ctx = bev_amd.BevContext(_p(), device=0, max_batch=8)
    try:
        offs, flat = _pack(frames)
        d_in, d_grids, d_energy = _dev(flat), guarded(n_db * ac.GRID * ac.GRID), guarded(4 * n_db)
        d_tab, d_best, d_det = guarded(2 * n * R), guarded(4 * n), guarded(2 * n * D)
        pick = np.array(ac.HAND_OVER)
        sub = np.ascontiguousarray(hits[pick])
        d_sub_tab = torch.zeros(2 * len(pick) * R, dtype=torch.uint8, device=d_in.device)
        d_sub_best = torch.zeros(4 * len(pick), dtype=torch.uint8, device=d_in.device)
        d_fine = {k: torch.zeros(len(pick) * R, dtype=torch.uint8, device=d_in.device) for k in ac.ITERATIONS}
        torch.cuda.synchronize()
        # the database's grids from the first seven frames of the same buffer, every hit, then the hand-over of HAND_OVER's hits:
        # their table straight into the fine call, no synchronisation in between
        ctx.align_grid_device(n_db, d_in.data_ptr(), offs[: n_db + 1], d_grids.data_ptr(), d_energy.data_ptr(), prm)
        ctx.align_hits_device(len(frames), d_in.data_ptr(), offs, n_db, d_grids.data_ptr(), d_energy.data_ptr(), hits, d_tab.data_ptr(),
                              d_best.data_ptr(), d_det.data_ptr(), prm)
        ctx.align_hits_device(len(frames), d_in.data_ptr(), offs, n_db, d_grids.data_ptr(), d_energy.data_ptr(), sub,
                              d_sub_tab.data_ptr(), d_sub_best.data_ptr(), 0, prm)
        for k in ac.ITERATIONS:
            ctx.fine_registration_device(len(frames), d_in.data_ptr(), offs, sub, d_fine[k].data_ptr(), d_sub_tab.data_ptr(),
                                         d_sub_best.data_ptr(), 0.2, gt.fixed_params(gt.FINE_D, k))
        ctx.synchronize()
        assert guard_ok(d_grids, n_db * ac.GRID * ac.GRID) and guard_ok(d_tab, 2 * n * R) and guard_ok(d_best, 4 * n) and guard_ok(d_det, 2 * n * D)
        grids = d_grids[: n_db * ac.GRID * ac.GRID].cpu().numpy().reshape(n_db, ac.GRID, ac.GRID)
        res = d_tab[: 2 * n * R].cpu().numpy().view(ICP_RESULT_DTYPE).reshape(n, 2)
        best = d_best[: 4 * n].cpu().numpy().view(np.int32)
        det = d_det[: 2 * n * D].cpu().numpy().view(ALIGN_DETAIL_DTYPE).reshape(n, 2)
        fine = {k: d_fine[k].cpu().numpy().view(ICP_RESULT_DTYPE) for k in ac.ITERATIONS}
        sub_tab = d_sub_tab.cpu().numpy().view(ICP_RESULT_DTYPE).reshape(-1, 2)
    finally:
        ctx.close()
    assert grids.tobytes() == want_grids.tobytes()
    assert res.tobytes() == want_res.tobytes() and best.tobytes() == want_best.tobytes() and det.tobytes() == want_det.tobytes()
    assert sub_tab.tobytes() == want_res[pick].tobytes()
    assert np.array_equal(best, S["flip"])
    for k in range(n):
        T = res[k, best[k]]["T"]
        e = np.abs(np.array([T[3], T[7]], np.float64) - S["shift"][k])
        assert (e <= ac.CELL).all(), (k, e)
    for i, k in enumerate(pick):
        tol = ac.tol(int(k))
        assert tol <= gt.CAP
        for it in ac.ITERATIONS:
            rec = fine[it][i]
            assert int(rec["converged"]) == 1 and int(rec["state"]) == gt.ICP_ITERATIONS and int(rec["iterations"]) == it, (k, it, rec)
            d = gt.dist(rec["T"], ac.trajectory(int(k))[it - 1])
            print(f"hit {k}, {it} iterations: {d:.1e} from the float64 reference, tol {tol:.1e}")
            assert d <= tol, (k, it, d, tol)
        print(f"hit {k}: {gt.dist(fine[max(ac.ITERATIONS)][i]['T'], S['T_true'][k]):.3f} from the truth after 8 iterations")
