"""The NumPy statement of the debug views (tests/debug_views_model.py) against itself, no GPU: the gather the device runs paints the
same image as the reference's ordered scatter, the stated summation order agrees with the plain serial sum, the defaults are what the
header says, and the cases hold the edges they were built for."""
import numpy as np
import pytest

import debug_views_model as dv

VARIANTS = {"defaults": (None, None), "custom": ("custom", "asymmetric")}


def _variant(name):
    cm, st = VARIANTS[name]
    return (None if cm is None else dv.custom_colormap()), (None if st is None else dv.asymmetric_stencil())


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(dv.CASES))
def test_gather_equals_painter(name, variant):
    """why a gather may replace the ordered scatter: the pixel's winner is the covering cell that comes last in raster order"""
    c = dv.case(name)
    colormap, stencil = _variant(variant)
    ids, wgt = c["planes"]
    got, M, cells = dv.keyframe_view(c["grey"], ids, wgt, 0.0, colormap, stencil)
    want, M2, cells2 = dv.keyframe_view(c["grey"], ids, wgt, 0.0, colormap, stencil, render=dv.render_painter)
    assert cells == cells2 == c["cells"] and M == M2
    assert got.tobytes() == want.tobytes()
    covered = (got != np.repeat(c["grey"][..., None], 3, axis=2)).any(axis=2).sum()
    assert covered >= cells * (0 if variant == "custom" else 1) and covered > 0


@pytest.mark.parametrize("name", list(dv.RANDOM_CASES))
def test_stated_order_agrees_with_serial_sum(name):
    ok, q = dv.quotients(*dv.case(name)["planes"])
    stated, serial = dv.stated_sum(q), dv.serial_sum(q[ok].tolist())
    assert abs(stated - serial) <= 1e-12 * abs(serial), (stated, serial)


def test_default_stencil_and_colormap():
    s = dv.default_stencil()
    assert s.shape == (7, 7) and int(s.sum()) == 29 and s[3, 3] == 1
    assert np.array_equal(s, s[::-1, ::-1])          # point-symmetric
    cm = dv.default_colormap()
    assert cm.shape == (256, 3) and cm.dtype == np.uint8
    assert tuple(cm[0]) == (128, 0, 0) and tuple(cm[255]) == (0, 0, 128) and cm[128][1] == 255
    a = dv.asymmetric_stencil()
    assert a[3, 3] and not any(np.array_equal(a, t) for t in (a[::-1], a[:, ::-1], a[::-1, ::-1], a.T, a.T[::-1], a.T[:, ::-1], a.T[::-1, ::-1]))


def test_frame_view_statement():
    g = np.array([[0, 127, 128, 255, 129, 200]], dtype=np.uint8)
    assert np.array_equal(dv.frame_view(g), np.repeat(g[..., None], 3, axis=2))
    masked = dv.frame_view(g, np.zeros_like(g))
    assert masked[0, :, 2].tolist() == [0, 127, 128, 255, 129, 200]
    assert masked[0, :, 0].tolist() == masked[0, :, 1].tolist() == [0, 0, 0, 127, 1, 72]
    half = dv.frame_view(g, np.array([[1, 0, 7, 0, 255, 0]], dtype=np.uint8))
    assert half[0, :, 0].tolist() == [0, 0, 128, 127, 129, 72]


def test_cases_hold_their_edges():
    """the tie case has at least 8 unrounded levels of exactly k + 1/2 with both parities, and rounds them to even; the range case clamps
    to 0 and 255 and skips the four cells that do not qualify; an empty map leaves M alone"""
    c = dv.case("ties")
    ids, wgt = c["planes"]
    _, M, cells = dv.keyframe_view(c["grey"], ids, wgt, 0.0)
    assert M == 255.0 / 64.0 and cells == 11
    ok, u = dv.unrounded_levels(ids, wgt, M)
    ties = u[ok][(u[ok] % 1.0 == 0.5) & (u[ok] < 255)]
    k = np.floor(ties).astype(int)
    assert len(ties) >= 8 and (k % 2 == 0).any() and (k % 2 == 1).any() and sorted(k.tolist()) == sorted(dv.TIE_LEVELS)
    lv = dv.levels(ids, wgt, M)
    assert sorted(lv[lv != dv.EMPTY].tolist()) == sorted([kk + (kk & 1) for kk in dv.TIE_LEVELS] + [255])
    c = dv.case("range")
    ids, wgt = c["planes"]
    _, M, cells = dv.keyframe_view(c["grey"], ids, wgt, 0.0)
    lv = dv.levels(ids, wgt, M)
    assert cells == 4 and (lv != dv.EMPTY).sum() == 4
    assert lv[5, 5] == 255 and lv[5, 15] == 0 and lv[5, 25] == 0 and lv[15, 5] == 0
    assert all(lv[15, x] == dv.EMPTY for x in (12, 17, 22, 27))
    z = np.zeros((9, 11))
    img, M, cells = dv.keyframe_view(dv.grey_image(11, 9), z, z, 3.5)
    assert M == 3.5 and cells == 0 and np.array_equal(img, np.repeat(dv.grey_image(11, 9)[..., None], 3, axis=2))
    # a NaN level (q = inf over M = inf) is 0
    ids, wgt = np.zeros((9, 11)), np.zeros((9, 11))
    ids[4, 5] = 1.0
    _, M, cells = dv.keyframe_view(dv.grey_image(11, 9), ids, wgt, 0.0)
    assert cells == 1 and np.isinf(M) and dv.levels(ids, wgt, M)[4, 5] == 0


def test_wrapper_exists():
    from dsopp_amd import capi
    assert hasattr(capi, "DebugViews")
    for name in ("frame", "frame_device", "keyframe", "keyframe_device", "keyframe_planes", "maximum_idepth"):
        assert hasattr(capi.DebugViews, name), name
    assert {s for s in capi.SYMBOLS if s.startswith("dsopp_hip_debug_views_")} >= {
        "dsopp_hip_debug_views_create", "dsopp_hip_debug_views_destroy", "dsopp_hip_debug_views_frame", "dsopp_hip_debug_views_keyframe"}
    # the host mirror names it too (tests/test_host_adapter.py compiles that header)
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mirror = open(os.path.join(root, "dsopp_amd", "host", "dsopp_hip_solvers.hpp")).read()
    assert "class HipDebugViews" in mirror and "maximumIdepth()" in mirror


def test_creation_needs_a_gpu():
    """there is no CPU path: without a device creation fails with DSOPP_HIP_ERR_HIP (-4)"""
    from dsopp_amd import capi
    if capi.device_count() > 0:
        v = capi.DebugViews(16, 8)
        v.close()
        return
    with pytest.raises(capi.HipError) as e:
        capi.DebugViews(16, 8)
    assert "-4" in str(e.value)
