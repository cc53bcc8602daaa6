"""The NumPy model of the device undistorter (tests/undistort_model.py) pinned on a hand-computed example and against an independent
bilinear interpolation, and what the library's new entry points do without a device.  What the GPU tests (test_gpu_undistort.py)
hold the device to is only as good as this model."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import undistort_model as um

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dsopp_hip_undistorter_create", "dsopp_hip_undistorter_destroy", "dsopp_hip_undistorter_sizes", "dsopp_hip_undistorter_undistort",
               "dsopp_hip_undistorter_undistort_device", "dsopp_hip_pyramid_build_undistorted", "dsopp_hip_feature_extractor_extract_from_pyramid")
ERR_INVALID_ARGUMENT, ERR_HIP = -1, -4


def test_hand_computed_3x3():
    """nine map entries worked out on paper (weights w = (32 - fx)(32 - fy) 32 etc., out = (sum + 16384) >> 15):
      (0, 0), (1, 0)       no fraction: copies 0 and 255
      (-1, -1)             the reference's failure marker: both axes reflect to 1 -> src[1, 1] = 50
      (2.5 / 32, 0)        a tie: rint(2.5) = 2, fx = 2:   (2 * 1024 * 255 + 16384) >> 15 = 538624 >> 15 = 16   (fx = 3 would give 24)
      (3.5 / 32, 0)        a tie: rint(3.5) = 4, fx = 4:   (4 * 1024 * 255 + 16384) >> 15 = 1060864 >> 15 = 32  (fx = 3 would give 24)
      (2.5, 2.5)           x taps 2 and reflect(3) = 1, the same in y: 8192 * (200 + 80 + 60 + 50) + 16384 = 3211264 -> 98
      (-0.5, 1)            sx = -16: floor -1, fx = 16; x taps reflect(-1) = 1 and 0: 16384 * (50 + 40) + 16384 = 1490944 -> 45
      (6, -5)              several periods out: 6 mod 4 = 2, -5 mod 4 = 3 -> 1: src[1, 2] = 60
      (1.25, 0.75)         fx = 8, fy = 24: 6144 * 255 + 2048 * 10 + 18432 * 50 + 6144 * 60 + 16384 = 2893824 -> 88"""
    src = np.array([[0, 255, 10], [40, 50, 60], [70, 80, 200]], dtype=np.uint8)
    map_x = np.array([[0, 1, -1], [2.5 / 32, 3.5 / 32, 2.5], [-0.5, 6, 1.25]], dtype=np.float32)
    map_y = np.array([[0, 0, -1], [0, 0, 2.5], [1, -5, 0.75]], dtype=np.float32)
    assert um.remap(src, map_x, map_y).tolist() == [[0, 255, 50], [16, 32, 98], [45, 60, 88]]


def test_ties_round_to_even_and_negative_coordinates_floor():
    k = np.arange(-8, 8)
    i, f = um.fixed_point(((k + 0.5) / 32).astype(np.float32))   # exactly representable: every one is a tie
    s = i * 32 + f
    assert (s % 2 == 0).all() and (np.abs(s - (k + 0.5)) == 0.5).all()
    assert um.fixed_point(np.float32(-1.0)) == (-1, 0)
    assert um.fixed_point(np.float32(-0.25)) == (-1, 24)
    assert um.fixed_point(np.float32(-2.5 / 32)) == (-1, 30)     # rint(-2.5) = -2
    assert um.fixed_point(np.float32(37.03125)) == (37, 1)


def test_reflect_101():
    assert um.reflect_101(np.arange(-7, 11), 4).tolist() == [1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2]
    assert um.reflect_101(np.arange(-3, 5), 2).tolist() == [1, 0, 1, 0, 1, 0, 1, 0]
    for n in (2, 3, 7):   # neighbours stay neighbours: the device table stores only the sign of x1 - x0
        r = um.reflect_101(np.arange(-50, 50), n)
        assert (np.abs(np.diff(r)) == 1).all() and r.min() == 0 and r.max() == n - 1


def test_identity_and_failure_marker():
    rng = np.random.default_rng(0)
    src = rng.integers(0, 256, (48, 64)).astype(np.uint8)
    mx, my = um.identity_maps(64, 48)
    assert np.array_equal(um.remap(src, mx, my), src)
    marker = np.full((3, 5), -1, dtype=np.float32)
    assert (um.remap(src, marker, marker) == src[1, 1]).all()


@pytest.mark.parametrize("sizes", [((64, 48), (64, 48)), ((80, 60), (67, 45)), ((2, 2), (5, 3))], ids=lambda s: f"{s[0]}to{s[1]}")
def test_model_against_scipy_bilinear(sizes):
    """an independent float bilinear interpolation with mirror borders.  The bound is derived: the coordinate is quantised to 1/32 by
    rounding, so each axis is off by at most 1/64 pixel, across which the interpolant changes by at most D/64 per axis where D is the
    largest difference between neighbouring source pixels (255 for uniform noise): D/32 in all, plus 0.5 for the final rounding."""
    from scipy.ndimage import map_coordinates
    (W, H), (w, h) = sizes
    rng = np.random.default_rng(W * 1000 + w)
    src = rng.integers(0, 256, (H, W)).astype(np.uint8)
    mx = rng.uniform(-3 * W, 4 * W, (h, w)).astype(np.float32)
    my = rng.uniform(-3 * H, 4 * H, (h, w)).astype(np.float32)
    want = map_coordinates(src.astype(np.float64), [my.astype(np.float64), mx.astype(np.float64)], order=1, mode="mirror")
    got = um.remap(src, mx, my).astype(np.float64)
    D = 255.0
    worst = np.abs(got - want).max()
    print(f"{sizes}: largest difference {worst:.3f} grey levels, bound {D / 32 + 0.5:.3f}")
    assert worst <= D / 32 + 0.5


def test_camera_maps_have_failures_and_a_fixed_centre():
    """the two camera maps the GPU tests use: the 4-pixel border fails (-1, -1), the principal ray maps to the principal point"""
    W, H = 64, 48
    for mx, my in (um.simple_radial_maps(W, H, 50.0, 31.5, 24.25, -0.2, 0.05), um.tum_fov_maps(W, H, 45.0, 44.0, 31.5, 24.25, 0.9)):
        assert mx.dtype == np.float32 and mx.shape == (H, W)
        failed = (mx == -1) & (my == -1)
        assert failed[:4].all() and failed[:, :4].all() and failed[-4:].all() and failed[:, -4:].all()
        assert not failed[8:-8, 8:-8].any()
        assert (mx[H // 2, W // 2], my[H // 2, W // 2]) == (31.5, 24.25)
        ok = ~failed
        assert (mx[ok] >= 4).all() and (mx[ok] <= W - 5).all() and (my[ok] >= 4).all() and (my[ok] <= H - 5).all()
        assert np.abs(mx - um.identity_maps(W, H)[0])[ok].max() > 0.5   # it does distort


def test_discs_drawn_at_distorted_points_appear_at_their_pinhole_pixels():
    """the reference's own undistorter test (test/test/sensors/camera/calibration/undistorter.cpp:91-137) on the model: a filled disc
    of radius 4 drawn where the distorted camera sees a ray is brighter than 100 at the pinhole projection of that ray"""
    W, H = 160, 120
    rng = np.random.default_rng(2)
    ys, xs = np.mgrid[0:H, 0:W]
    for mx, my in (um.simple_radial_maps(W, H, 120.0, 79.5, 60.25, -0.2, 0.05), um.tum_fov_maps(W, H, 110.0, 108.0, 79.5, 60.25, 0.9)):
        for _ in range(10):
            u, v = int(rng.integers(20, W - 20)), int(rng.integers(20, H - 20))
            assert mx[v, u] != -1
            src = np.where((xs - int(mx[v, u])) ** 2 + (ys - int(my[v, u])) ** 2 <= 16, 255, 0).astype(np.uint8)
            assert um.remap(src, mx, my)[v, u] > 100


def test_new_symbols_declared_and_exported():
    from dsopp_amd import capi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dsopp_hip.h")).read(), flags=re.S)
    lib = C.CDLL(capi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/dsopp_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in capi.SYMBOLS


def _create(in_w, in_h, out_w, out_h, map_x, map_y):
    from dsopp_amd import capi
    h = C.c_void_p()
    ptr = lambda m: None if m is None else m.ctypes.data_as(C.c_void_p)
    return capi.lib().dsopp_hip_undistorter_create(0, None, in_w, in_h, out_w, out_h, ptr(map_x), ptr(map_y), C.byref(h))


def test_create_refuses_bad_arguments_before_any_device_is_touched():
    mx, my = um.identity_maps(8, 6)
    assert _create(1, 6, 8, 6, mx, my) == ERR_INVALID_ARGUMENT
    assert _create(8, 1, 8, 6, mx, my) == ERR_INVALID_ARGUMENT
    assert _create(8, 6, 8, 6, mx, None) == ERR_INVALID_ARGUMENT
    assert _create(8, 6, 8, 6, None, my) == ERR_INVALID_ARGUMENT
    assert _create(8, 6, 7, 6, None, None) == ERR_INVALID_ARGUMENT      # the identity cannot change the size
    for bad in (np.nan, np.inf, -np.inf, 2.0 ** 20 + 1, -(2.0 ** 20) - 1):
        for which in (0, 1):
            maps = [mx.copy(), my.copy()]
            maps[which][5, 7] = bad
            assert _create(8, 6, 8, 6, *maps) == ERR_INVALID_ARGUMENT, (bad, which)


def test_no_cpu_fallback():
    """without a device every new entry point that computes fails with DSOPP_HIP_ERR_HIP"""
    from dsopp_amd import capi
    if capi.device_count() > 0:
        pytest.skip("a GPU is present")
    mx, my = um.identity_maps(8, 6)
    assert _create(8, 6, 8, 6, mx, my) == ERR_HIP
    assert _create(8, 6, 8, 6, None, None) == ERR_HIP
    edge = np.full((6, 8), 2.0 ** 20, dtype=np.float32)   # the largest coordinate allowed is not refused as an argument
    assert _create(8, 6, 8, 6, edge, -edge) == ERR_HIP
    with pytest.raises(capi.HipError) as e:
        capi.Undistorter((8, 6), (8, 6), mx, my)
    assert "-4" in str(e.value)
