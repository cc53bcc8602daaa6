"""The reference depth maps (splat, pools, dilation: depth_map_kernels.hpp), the row scan that turns a level into reference points
(align.hip) and the three optical-flow kernels, against the NumPy statement of tests/depth_maps_model.py on the cases of its table: exact
inputs ON every decision edge, sizes that are no multiple of any tile, a full splat batch, more than 256 partial blocks and more than
65 536 reference points.  The windows are loaded and NOT solved: the model reads exactly what the kernels read, so the only difference
left is the order of the atomic additions — the 1e-12 bar tests/test_depth_maps.py holds a refill against a creation to."""
import numpy as np
import pytest

import depth_maps_model as dm
from dsopp_amd import synthetic as syn

pytestmark = pytest.mark.gpu

ORDER_ONLY = 1e-12


def _pixelinfo(c, i):
    """a constant image; for the cases whose variances are read back a seeded random one, so that H_dd differs from landmark to landmark"""
    if c["variance"] == "readback":
        plane = np.random.default_rng(c["image_seed"] + i).integers(0, 256, (c["H"], c["W"])).astype(np.float64)
    else:
        plane = np.full((c["H"], c["W"]), 100.0)
    return syn.pixelinfo_from_plane(plane)


def _load(c, capi):
    g = capi.HipWindow(capi.default_pba_options(estimate_uncertainty=1 if c["variance"] == "readback" else 0))
    newest = len(c["poses"]) - 1
    for i, T in enumerate(c["poses"]):
        g.push_frame(i, 1000 * (i + 1), _pixelinfo(c, i), None, c["intr"], T, 1.0, np.zeros(2), i == 0, False)
        s = c["sources"][i] if i < newest else dict(uv=np.zeros((0, 2)), idepth=np.zeros(0), flags=np.zeros(0, dtype=np.uint8))
        g.set_landmarks(i, s["uv"], s["idepth"], np.zeros((len(s["idepth"]), 8)), s["flags"])
    for i, s in enumerate(c["sources"]):
        if len(s["idepth"]):
            g.set_connection(i, newest, s["status"])
    if c["variance"] == "readback":
        g.begin()
        g.linearize()
        g.calculate_step(1e-5)
    return g


def _model(c, g, flags=None):
    """the model's (levels, Splat) of what the window holds: the case's own inputs, or — where the variances are the window's — everything
    the splat reads, taken from the HIP window's getters"""
    if c["variance"] != "readback":
        return dm.case_maps(c, flags=flags)
    newest = len(c["poses"]) - 1
    lms = [g.get_landmarks(i, with_hpib=False) for i in range(newest)]
    for lm in lms:
        assert np.all(np.isfinite(lm["inv_hdd"]))
    assert len(np.unique(np.concatenate([lm["inv_hdd"] for lm in lms]))) > 100      # (a textured image: the weights differ)
    return dm.case_maps(c, variances=[lm["inv_hdd"] for lm in lms], flags=[lm["flags"] for lm in lms], idepths=[lm["idepth"] for lm in lms],
                        statuses=[g.get_residuals(i, newest)["status"] for i in range(newest)], poses=[g.get_pose(i)[0] for i in range(newest + 1)])


def _assert_maps(maps, want, tag):
    for lvl, (wi, ww) in enumerate(want):
        ids, wgt = maps.get_level(lvl)
        assert ids.shape == wi.shape, (tag, lvl)
        assert np.array_equal(wgt > 0, ww > 0), (tag, lvl, int(((wgt > 0) != (ww > 0)).sum()))
        ew, ei = np.abs(wgt - ww).max(), np.abs(ids - wi).max()
        print(f"{tag} level {lvl}: weight error {ew:.3e} of {np.abs(ww).max():.3e}, idepth-sum error {ei:.3e} of {np.abs(wi).max():.3e}")
        assert ew <= ORDER_ONLY * np.abs(ww).max(), (tag, lvl)
        assert ei <= ORDER_ONLY * np.abs(wi).max(), (tag, lvl)


def _assert_flow(c, maps, levels, tag):
    """the measure of every listed level under the four transforms against the model and the oracle on the planes the device holds;
    a batch of one equals the same entry of the batch of four bit for bit; a level without a pixel gives NaN on all sides"""
    from oracle import pyoracle as po
    Ts = dm.flow_transforms()
    params = [syn.mat_to_params(T) for T in Ts]
    out = {}
    for lvl in levels:
        intr = c["intr"] / (1 << lvl)
        ids, wgt = maps.get_level(lvl)
        got = maps.mean_square_optical_flow(lvl, intr, params)
        for k, T in enumerate(Ts):
            want, n = dm.flow(ids, wgt, intr, T)
            ref = po.mean_square_optical_flow(ids, wgt, intr, params[k])
            print(f"{tag} level {lvl} transform {k}: {got[k]!r} model {want!r} oracle {ref!r} over {n} pixels")
            assert dm.same_or_both_nan(got[k], want, ORDER_ONLY * max(want, 1e-3)), (tag, lvl, k, got[k], want)
            assert dm.same_or_both_nan(got[k], ref, ORDER_ONLY * max(ref, 1e-3)), (tag, lvl, k, got[k], ref)
        one = maps.mean_square_optical_flow(lvl, intr, [params[1]])
        assert one.tobytes() == got[1:2].tobytes(), (tag, lvl)
        out[lvl] = got
    return out


@pytest.mark.parametrize("name", list(dm.CASES))
def test_maps_flow_and_refill(name):
    from dsopp_amd import capi
    c = dm.case(name)
    L = c["levels"]
    g = _load(c, capi)
    maps = g.create_reference_depth_maps(L)
    want, s = _model(c, g)
    assert s.exact if c["kind"] == "exact" else s.ambiguous == 0
    _assert_maps(maps, want, f"{name} created")
    first = [maps.get_level(l) for l in range(L)]
    if c["kind"] == "exact" and c["variance"] == "constant":
        # no contribution lost or doubled: an occupied cell (the dilation leaves those alone) holds the hit count times the one weight
        hits = first[0][1] / dm.weights(dm.CONSTANT_VARIANCE)
        assert np.abs(hits - s.k)[s.k > 0].max() <= 1e-12
    # the dense pass: no aligner has touched these maps
    _assert_flow(c, maps, range(L), f"{name} dense")
    with pytest.raises(capi.HipError):
        maps.mean_square_optical_flow(0, c["intr"], [syn.mat_to_params(np.eye(4))] * 5)
    # refill with the largest source switched off: nothing of the previous fill survives in the temporaries.  (set_landmarks moves only the
    # marginalised bit of a landmark the window already holds — the outlier bit of those lives on the device — so the source's landmarks
    # are handed over as marginalised outliers, flags 3)
    off = int(np.argmax([len(x["idepth"]) for x in c["sources"]]))
    src = c["sources"][off]
    n = len(src["idepth"])
    g.set_landmarks(off, src["uv"], src["idepth"], np.zeros((n, 8)), np.full(n, 3, dtype=np.uint8))
    g.refill_reference_depth_maps(maps)
    reduced, s2 = _model(c, g, flags=[np.full(len(x["idepth"]), 3, dtype=np.uint8) if i == off else x["flags"] for i, x in enumerate(c["sources"])])
    assert s2.k.sum() < s.k.sum()
    _assert_maps(maps, reduced, f"{name} reduced")
    # ... and back: equal to the first creation up to the order of the atomic additions
    g.set_landmarks(off, src["uv"], src["idepth"], np.zeros((n, 8)), src["flags"])
    g.refill_reference_depth_maps(maps)
    for l in range(L):
        a, b = maps.get_level(l)
        assert np.array_equal(b > 0, first[l][1] > 0), l
        assert np.abs(a - first[l][0]).max() <= ORDER_ONLY * np.abs(a).max() and np.abs(b - first[l][1]).max() <= ORDER_ONLY * np.abs(b).max(), l
    _assert_maps(maps, want, f"{name} refilled")
    _assert_flow(c, maps, range(L), f"{name} dense after refill")
    maps.close()
    g.close()


def _bits(r):
    return {k: np.asarray(v).tobytes() for k, v in r.items()}


@pytest.mark.parametrize("name,levels", [("edges", (0, 2, 4)), ("half", (0, 1)), ("tall", (0, 1)), ("capacity", (0,))],
                         ids=["edges", "half", "tall", "capacity"])
def test_reference_points_and_point_flow(name, levels):
    """the device scan of a level against the model's point list (count) and against the host scan of the downloaded planes (the solve,
    field for field and bit for bit: that pins the list's order and contents); then the flow over that list; then, after a refill, the
    dense pass again"""
    from dsopp_amd import capi
    c = dm.case(name)
    W, H, L = c["W"], c["H"], c["levels"]
    g = _load(c, capi)
    maps = g.create_reference_depth_maps(L)
    want, _ = _model(c, g)
    rng = np.random.default_rng(7)
    pyr, tgt = capi.Pyramid(W, H, L), capi.Pyramid(W, H, L)
    pyr.build(rng.integers(0, 256, (H, W)).astype(np.uint8))
    tgt.build(rng.integers(0, 256, (H, W)).astype(np.uint8))
    T_ref = c["poses"][-1]
    T_init = syn.mat_to_params(syn.params_to_mat(T_ref) @ syn.se3_exp(np.array([0.01, -0.006, 0.004, 0.002, -0.001, 0.003])))
    dense = _assert_flow(c, maps, levels, f"{name} dense")
    for lvl in range(L):
        intr = c["intr"] / (1 << lvl)
        n_model = len(dm.reference_points(*want[lvl]))
        a = capi.HipAligner(capi.default_align_options())
        a.reset()
        a.push_reference_depth_maps(5000, T_ref, pyr, lvl, intr, maps, 1.0, np.zeros(2))
        assert a.num_points() == n_model, (lvl, a.num_points(), n_model)
        if lvl in levels:
            a.push_target(6000, T_init, tgt, lvl, intr, 1.0, np.zeros(2))
            r_dev = a.solve()
            a.close()
            ids, wgt = maps.get_level(lvl)
            a = capi.HipAligner(capi.default_align_options())
            a.reset()
            a.push_reference_depth_map(5000, T_ref, pyr, lvl, intr, ids, wgt, 1.0, np.zeros(2))
            assert a.num_points() == n_model
            a.push_target(6000, T_init, tgt, lvl, intr, 1.0, np.zeros(2))
            r_host = a.solve()
            print(f"{name} level {lvl}: {n_model} points, {r_dev['iterations']} iterations, n_valid {r_dev['n_valid']}, energy {r_dev['energy']!r}")
            assert r_dev["n_valid"] == r_host["n_valid"] and r_dev["iterations"] == r_host["iterations"]
            assert _bits(r_dev) == _bits(r_host), lvl
        a.close()
    if "min_points" in c:
        assert len(dm.reference_points(*want[0])) > 65536     # more than 256 workgroups of the point-list kernel
    # every level's points are extracted now: the measure walks the lists — the same pixels, so the same number up to summation order
    points = _assert_flow(c, maps, levels, f"{name} points")
    for lvl in levels:
        for k in range(4):
            assert dm.same_or_both_nan(points[lvl][k], dense[lvl][k], ORDER_ONLY * max(dense[lvl][k], 1e-3)), (lvl, k)
    # a refill makes the lists stale: the dense pass again, on planes equal to the first ones up to the order of the atomic additions
    g.refill_reference_depth_maps(maps)
    _assert_maps(maps, want, f"{name} refilled")
    _assert_flow(c, maps, levels, f"{name} dense after refill")
    for obj in (maps, pyr, tgt, g):
        obj.close()


def test_refusals():
    """a level below 3 pixels is refused, and so are 0 and 6 levels; the window goes on to create what it can"""
    from dsopp_amd import capi
    W = H = 20
    rng = np.random.default_rng(3)
    cells = dm._roi_cells(W, H)
    c = dict(kind="exact", W=W, H=H, levels=2, intr=dm._exact_intr(W, H), poses=[dm._pose((0, 0, 0))] * 3, variance="constant",
             sources=[dm._source(cells[rng.permutation(len(cells))[:40]], dm._dyadic_idepth(40, rng)), dm._source(cells[::5], dm._dyadic_idepth(len(cells[::5]), rng))])
    g = _load(c, capi)
    for levels in (5, 0, 6):      # 20 -> 10 -> 5 -> 2: level 3 is too small
        with pytest.raises(capi.HipError):
            g.create_reference_depth_maps(levels)
    maps = g.create_reference_depth_maps(2)
    want, s = _model(c, g)
    assert s.exact and (s.k > 0).sum() > 40
    _assert_maps(maps, want, "20 x 20")
    _assert_flow(c, maps, range(2), "20 x 20")
    maps.close()
    g.close()
