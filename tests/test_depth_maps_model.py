"""The NumPy statement of the reference depth maps (tests/depth_maps_model.py) against the CPU oracle and against the loop statement of
tests/test_depth_maps.py, on every case of the table the GPU tests use; the conditions the cases are built to meet; and three 5 x 5 inputs
written out by hand that pin the dilation rules directly."""
import time

import numpy as np
import pytest

import depth_maps_model as dm
from test_depth_maps import _numpy_depth_maps, _numpy_flow

NAMES = list(dm.CASES)
LOOP_NAMES = [n for n in NAMES if dm.case(n)["W"] * dm.case(n)["H"] <= 77 * 59]


def _close(got, want, rel):
    return np.abs(got - want).max() <= rel * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("name", NAMES)
def test_model_matches_oracle(name):
    from oracle import pyoracle as po
    from dsopp_amd import synthetic as syn
    c = dm.case(name)
    maps, s = dm.constant_variance_maps(name)
    want = po.create_reference_depth_maps(dm.oracle_sources(dm.model_sources(c)), c["poses"][-1], c["intr"], c["W"], c["H"], c["levels"])
    assert [m[0].shape[::-1] for m in maps] == dm.level_sizes(c["W"], c["H"], c["levels"])
    for lvl, ((a, b), (wa, wb)) in enumerate(zip(maps, want)):
        assert a.shape == wa.shape
        assert np.array_equal(b > 0, wb > 0), lvl
        assert _close(b, wb, 1e-12), lvl
        assert _close(a, wa, 1e-9), lvl
        intr = c["intr"] / (1 << lvl)
        for k, T in enumerate(dm.flow_transforms()):
            got, n = dm.flow(a, b, intr, T)
            ref = po.mean_square_optical_flow(a, b, intr, syn.mat_to_params(T))
            assert dm.same_or_both_nan(got, ref, 1e-12 * max(ref, 1e-3) if n else 0.0), (lvl, k, got, ref, n)
            assert dm.same_or_both_nan(got, dm.flow(a, b, intr, syn.mat_to_params(T))[0], 1e-13), (lvl, k)   # 4 x 4 or 7-vector: the same pose
            if k == 2 and n:
                assert got < 1e-12     # identity: no flow


@pytest.mark.parametrize("name", LOOP_NAMES)
def test_model_matches_loop_statement(name):
    c = dm.case(name)
    maps, _ = dm.constant_variance_maps(name)
    want = _numpy_depth_maps(dm.oracle_sources(dm.model_sources(c)), c["poses"][-1], c["intr"], c["W"], c["H"], c["levels"])
    for lvl, ((a, b), (wa, wb)) in enumerate(zip(maps, want)):
        assert np.array_equal(b > 0, wb > 0), lvl
        assert _close(b, wb, 1e-12) and _close(a, wa, 1e-9), lvl
    a, b = maps[0]
    for k, T in enumerate(dm.flow_transforms()):
        got, n = dm.flow(a, b, c["intr"], T)
        if n:
            want_flow, want_n = _numpy_flow(a, b, c["intr"], T)
            assert n == want_n and abs(got - want_flow) <= 1e-12 * max(want_flow, 1e-3), (k, got, want_flow)


@pytest.mark.parametrize("name", NAMES)
def test_case_conditions(name):
    c = dm.case(name)
    t0 = time.perf_counter()
    maps, s = dm.case_maps(c)
    pts = [dm.reference_points(a, b) for a, b in maps]
    took = time.perf_counter() - t0
    assert took < 1.0, took                    # vectorised: the 10^5-cell cases well under a second
    assert len(c["sources"]) <= 15 and max(len(x["idepth"]) for x in c["sources"]) > 0
    if c["kind"] == "exact":
        assert s.exact
    else:
        assert s.ambiguous == 0
    assert (s.k > 0).sum() > 0 and np.array_equal(s.k > 0, s.wgt > 0)
    if c["variance"] == "constant":           # every contribution once: the weight plane is the hit count times the one weight
        assert np.abs(s.wgt / dm.weights(dm.CONSTANT_VARIANCE) - s.k).max() <= 1e-12 * s.k.max()
    if c.get("hits_once"):
        assert s.k.max() == 1 and s.k.sum() == sum(len(x["idepth"]) for x in c["sources"])
    if "min_points" in c:
        assert len(pts[0]) >= c["min_points"]
    # a reference point list is row-major, inside the border, and as long as the flow's pixel count under the identity
    for lvl, (p, (a, b)) in enumerate(zip(pts, maps)):
        if len(p):
            key = p[:, 1] * a.shape[1] + p[:, 0]
            assert np.all(np.diff(key) > 0) and p[:, 0].min() >= 4 and p[:, 0].max() <= a.shape[1] - 5 and p[:, 1].min() >= 4 and p[:, 1].max() <= a.shape[0] - 5
        assert dm.flow(a, b, c["intr"] / (1 << lvl), np.eye(4))[1] <= len(p)


def test_edges_case_is_as_designed():
    c = dm.case("edges")
    maps, s = dm.constant_variance_maps("edges")
    W, H = c["W"], c["H"]
    want = np.zeros((H, W), dtype=np.int64)
    for (x, y), k in c["expect"].items():
        want[y, x] = k
    assert np.array_equal(s.k, want)
    assert s.k[30, 40] == 64 and s.k[40, 50] == 2 and c["stacked"] == ((40, 30), 64)
    assert s.ambiguous == 4 + 2 + 1   # the landmarks ON a border, ON a tie and at z = 0 are there (and decided alike by all: the case is exact)
    for x, y in ((4, 4), (W - 5, 4), (4, H - 5), (W - 5, H - 5), (W - 5, 26), (26, H - 5), (4, 30), (30, 4), (11, 11), (16, 16), (54, 38)):
        assert s.k[y, x] == 1, (x, y)
    for x, y in ((4, 24), (24, 4), (W - 5, 28), (28, H - 5), (10, 11), (16, 15), (30, 36), (33, 36)):   # dropped, or rounded elsewhere
        assert s.k[y, x] == 0, (x, y)
    w1 = dm.weights(dm.CONSTANT_VARIANCE)
    assert abs(s.ids[38, 54] - 0.25 / 0.5 * w1) <= 1e-12 * w1    # depth scale 1 / 2
    # a cell with weight and a zero idepth sum: the splat keeps it, the scan and the flow drop it
    pts = dm.reference_points(*maps[0])
    for x, y in c["zero_sum_cells"]:
        assert s.wgt[y, x] > 0 and s.ids[y, x] == 0 and not np.any((pts[:, 0] == x) & (pts[:, 1] == y))
    assert np.any((pts[:, 0] == 23) & (pts[:, 1] == 8))          # idepth 1009 is a point
    # the isolated cell: its diagonal neighbours fill on levels 0 and 1, its axis neighbours do not
    x, y = c["isolated"]
    for lvl in (0, 1):
        b, xx, yy = maps[lvl][1], x >> lvl, y >> lvl
        assert b[yy, xx] > 0
        assert all(b[yy + oy, xx + ox] == b[yy, xx] for ox, oy in dm.DIAGONAL)
        assert all(b[yy + oy, xx + ox] == 0 for ox, oy in dm.AXIS)


def test_density_and_size_conditions():
    occupancy = {}
    for name in ("sparse", "half", "full"):
        c = dm.case(name)
        _, s = dm.constant_variance_maps(name)
        occupancy[name] = (s.k > 0).sum() / float((c["W"] - 8) * (c["H"] - 8))
    assert 0.005 < occupancy["sparse"] < 0.02 and 0.45 < occupancy["half"] < 0.55 and occupancy["full"] == 1.0
    maps, s = dm.constant_variance_maps("full")
    inner = np.zeros(s.k.shape, dtype=bool)
    inner[4:-4, 4:-4] = True
    assert np.array_equal(maps[0][1][inner], s.wgt[inner])          # level 0: nothing to fill inside the ROI
    assert not maps[2][1][0, :].any() and all(m[1][0, :].all() and m[1][:, -1].all() for m in maps[3:])   # from 6 x 6 on the border cells carry weight ...
    assert maps[4][0].shape == (3, 3) and maps[4][1].all()          # ... down to the 3 x 3 level
    assert [len(x["idepth"]) for x in dm.case("ragged")["sources"]] == [0, 1, 255, 256, 257, 700]
    # the tall case: 258 strips of 16 rows, with flow pixels in the strips past the 256th, and at least 100 of them per transform that sees any
    c = dm.case("tall")
    maps, s = dm.constant_variance_maps("tall")
    assert (c["H"] + 15) // 16 == 258 and (c["H"] + 255) // 256 == 17
    assert (s.k[4096:] > 0).sum() >= 100
    counts = [dm.flow(*maps[0], c["intr"], T)[1] for T in dm.flow_transforms()]
    assert min(counts[:3]) >= 100, counts
    c = dm.case("capacity")
    maps, s = dm.constant_variance_maps("capacity")
    assert len(c["sources"]) == 15 and (s.k > 0).sum() >= 66000 and len(dm.reference_points(*maps[0])) > 65536


def test_dilation_by_hand():
    """planes are indexed [y, x]; offsets are (dx, dy)"""
    z = np.zeros((5, 5))
    w, i = z.copy(), z.copy()
    w[1, 1], w[3, 3], w[1, 3] = 2.0, 4.0, 6.0      # three diagonal neighbours of the centre: (x, y) = (1, 1), (3, 3), (3, 1)
    i[1, 1], i[3, 3], i[1, 3] = 1.0, 3.0, 8.0
    w[2, 1], i[2, 1] = 100.0, 100.0                 # an axis neighbour of the centre: (x, y) = (1, 2)
    # 1. level 1, the diagonal rule: the centre takes the mean of its three weighted diagonal neighbours, in both planes
    oi, ow = dm.dilate_level(i, w, 1)
    assert oi[2, 2] == (3.0 + 1.0 + 8.0) / 3 and ow[2, 2] == (4.0 + 2.0 + 6.0) / 3
    assert ow[1, 2] == 100.0 and ow[3, 2] == 100.0 and oi[1, 2] == 100.0     # (2, 1) and (2, 3) see (1, 2) diagonally
    assert ow[2, 3] == 0      # (3, 2): two AXIS neighbours with weight, no diagonal one
    assert ow[3, 1] == 0      # (1, 3): its one candidate is the centre, filled in this very pass — neighbours are read from the undilated planes
    assert np.array_equal(ow[w > 0], w[w > 0]) and np.array_equal(oi[w > 0], i[w > 0])
    # 2. level 2, the axis rule, on the same planes
    oi, ow = dm.dilate_level(i, w, 2)
    assert oi[2, 2] == 100.0 and ow[2, 2] == 100.0                            # the centre sees (1, 2) alone
    assert ow[1, 2] == (6.0 + 2.0) / 2 and oi[1, 2] == (8.0 + 1.0) / 2        # (2, 1): right (3, 1) and left (1, 1)
    assert ow[2, 3] == (4.0 + 6.0) / 2 and oi[2, 3] == (3.0 + 8.0) / 2        # (3, 2): below (3, 3) and above (3, 1)
    assert ow[3, 1] == 100.0                                                  # (1, 3): above it lies (1, 2)
    assert dm.dilate_level(i, w, 0)[1].tolist() == dm.dilate_level(i, w, 1)[1].tolist() and dm.dilate_level(i, w, 3)[1].tolist() == ow.tolist()
    # ... and the reference's offset order, which shows in the rounding: (1, 1), (-1, -1), (1, -1), (-1, 1) sums 1e16 + 1 - 1e16 to 0
    i2 = i.copy()
    i2[3, 3], i2[1, 1], i2[1, 3] = 1e16, 1.0, -1e16
    assert dm.dilate_level(i2, w, 1)[0][2, 2] == 0.0
    # 3. border cells are never filled, on either rule, and occupied cells are never changed
    w = np.ones((5, 5))
    w[0, :] = w[-1, :] = w[:, 0] = w[:, -1] = 0
    w[2, 2] = 0
    for lvl in (0, 1, 2, 3):
        oi, ow = dm.dilate_level(w * 3.0, w, lvl)
        assert not ow[0, :].any() and not ow[-1, :].any() and not ow[:, 0].any() and not ow[:, -1].any()
        assert ow[2, 2] == 1.0 and oi[2, 2] == 3.0 and np.array_equal(ow[1:-1, 1:-1], np.ones((3, 3)))


def test_pool_by_hand():
    a = np.arange(35, dtype=np.float64).reshape(5, 7)       # odd sizes: the last row and column have no parent
    (p0, _), (p1, _), (p2, _) = dm.pool(a, a, 3)
    assert p1.shape == (2, 3) and p2.shape == (1, 1)
    assert p1[0, 0] == 0 + 1 + 7 + 8 and p1[1, 2] == 18 + 19 + 25 + 26 and p2[0, 0] == p1[:2, :2].sum()
