"""CPU: what can be established without a device about the world of raster_world_cases.py and about the checker the raster
family is tested against byte for byte: the filter's conditions, the oracle's composition against a float64
reference that rasters world coordinates, and mutants of that composition, each of which the reference catches."""
import numpy as np
import pytest

import raster_world_cases as rw
import raster_world_checker as ck

F64 = np.float64
SENSORS = tuple(rw.CONFIGS)
COMPARED = tuple(rw.maps())


@pytest.mark.parametrize("sensor", SENSORS)
def test_filter_conditions(sensor):
    c = rw.case(sensor)
    ck.params(c)                                                   # the configuration is the sensor's
    share = float(c.drop[c.seen].mean())
    print(f"{sensor}: {int(c.drop[c.seen].sum())} of {len(c.seen)} seen world points dropped ({100 * share:.1f} %)")
    assert 0 < share <= 0.10
    assert all(2048 < len(f) <= 3072 for f in c.frames), [len(f) for f in c.frames]     # three workgroups of 1024 each
    for f in c.frames:
        assert np.abs(np.c_[f["x"], f["y"], f["z"]]).max() < RANGE_BOUND
    reached, occupied = np.zeros(rw.N_LAYERS, bool), np.zeros(rw.N_LAYERS, bool)
    for name in COMPARED:
        full_multi, full_single = c.reference(name, keep_dropped=True)
        multi, single = c.reference(name)
        full_cells, now = rw.occupied(c, name, keep_dropped=True), rw.occupied(c, name)
        cells, lost = int(full_cells.sum()), int((full_cells & ~now).sum())
        if name in rw.SUBMAPS:
            print(f"{sensor} map {name}: {cells} occupied cells, {lost} lost all their points")
        assert cells > 0 and lost <= 0.10 * cells, (name, cells, lost)
        reached |= full_multi.any(axis=(1, 2))
        occupied |= multi.any(axis=(1, 2))
        # no point left within MARGIN of an edge, in any compared map
        assert not rw.near_edge(c.points(name, skip_label0=False), c.height_res, c.interval).any(), name
    assert reached.sum() >= 10 and np.array_equal(reached, occupied), (reached, occupied)
    print(f"{sensor}: layers reached and occupied: {np.flatnonzero(occupied).tolist()}")


RANGE_BOUND = 64.0   # MARGIN's derivation: a frame's coordinates stay below 64 m (the matrix entries' rounding times that)


def test_labels_and_general_matrices():
    c = rw.case("HDL_64E")
    for name in ("A", "B", "K", "T"):
        frames = [f for f, _ in c.maps[name]]
        seen = np.unique(np.concatenate([c.ids[f] for f in frames]))
        zero_in = np.array([sum(int(i in set(c.ids[f][c.labels[f] == 0].tolist())) for f in frames) for i in seen.tolist()])
        seen_in = np.array([sum(int(i in set(c.ids[f].tolist())) for f in frames) for i in seen.tolist()])
        always, some = int(((zero_in == seen_in) & (seen_in >= 2)).sum()), int(((zero_in > 0) & (zero_in < seen_in)).sum())
        print(f"map {name}: {always} points with label 0 in every entry (of two or more), {some} in some entries only")
        assert always >= 50 and some >= 50
    for name in ("T", "F", "G"):
        m = np.array([mat for _, mat in c.entries(name)], F64).reshape(-1, 3, 4)
        assert np.abs(m[:, :, :3]).min() > 0.01 and np.abs(np.abs(m) - 1).min() > 0.01 and np.abs(m[:, :, 3]).min() > 0.01, name
        assert np.abs(m[:, :2, 2]).max() * 2.0 > 0.25 and np.abs(m[:, 2, :2]).max() * 20.0 > 1.0     # z mixes in, and x, y into z
    lo = hi = 0
    for name in ("F", "G"):
        share, low, high = rw.off_image_share(c, name)
        print(f"map {name}: {100 * share:.1f} % of its points off the image ({low} on the low side of x, {high} on the high side)")
        assert 0.20 <= share <= 0.80
        lo, hi = lo + low, hi + high
    assert lo > 100 and hi > 100
    # D names frame 3 twice, under two matrices
    (f0, m0), (f1, m1) = c.entries("D")
    assert f0 == f1 == 3 and not np.array_equal(m0, m1)
    # the posed grids' matrices: general for k = 1, 2; every CLI pose is what the tool's row gives
    assert np.abs(c.posed_matrices()[:, 1:, :].reshape(-1, 3, 4)[:, :, :3]).min() > 0.01
    for k, row in enumerate(rw.CLI_POSES):
        want = rw.yaw_translate(*row)[:3].reshape(12)
        assert np.abs(c.entries(("cli", k))[0][1].astype(F64) - want).max() < 1e-5


@pytest.mark.parametrize("sensor", SENSORS)
def test_the_checker_composition_equals_the_float64_world(sensor):
    c = rw.case(sensor)
    tol = c.tol()
    assert 0 < tol <= rw.CAP, tol
    worst = 0.0
    for name in COMPARED:
        worst = max(worst, ck.compare(ck.composition(c, c.entries(name)), ck.reference(c, name), tol, f"{sensor}, map {name}"))
    print(f"{sensor}: 0 bytes differ in {2 * len(COMPARED)} uint8 images; float grids within {worst:.2e} of the float64 world, tol {tol:.2e}")
    assert ck.reference(c, "A")["multi"].any() and ck.reference(c, "F")["float0"].any()
    # label 0 matters, and the two float grids differ by it
    assert not np.array_equal(ck.reference(c, "A")["float1"], ck.reference(c, "A")["float0"])


@pytest.mark.parametrize("mutant", tuple(ck.MUTANTS))
@pytest.mark.parametrize("sensor", SENSORS)
def test_the_reference_catches_the_mutant(sensor, mutant):
    """Each mutant of the checker's construction must change at least 100 bytes of each image it can change, of every
    multi-entry map it can change (a float grid's cell counts as 4 bytes once it moves by more than tol).

    The world of ground_truth_cases.py alone misses that bar in six of the 33 cases (its ground lies below layer 0 and is 0 or
    1 in the uint8 image, two wall records share a byte of the 24-layer image, and at 2 m cells a map's uint8 image has 70 to
    270 non-zero bytes in all), so raster_world_cases.py adds posts and lamps to it and makes the lamps the class with label 0;
    the smallest count is then 100 (the last entry alone, OS1_64)."""
    c = rw.case(sensor)
    tol = c.tol()
    short, maps_changed = [], 0
    for name in rw.MULTI_ENTRY:
        images = ck.MUTANTS[mutant](c, name)
        if images is None:
            continue
        maps_changed += 1
        want = ck.reference(c, name)
        counts = {key: int(np.count_nonzero(np.abs(got.astype(F64) - want[key]) > tol)) * got.itemsize for key, got in images.items()}
        print(f"{sensor}, map {name}, {mutant}: bytes changed {counts}")
        if min(counts.values()) < 100:
            short.append((name, counts))
    assert maps_changed >= len(rw.MULTI_ENTRY) - 1
    assert not short, (sensor, mutant, short)
