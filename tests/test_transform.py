"""The NumPy model of the device image transformer (tests/transform_model.py) against closed forms, and what the library's new entry
points do without a device: the calibration and the argument errors.  What the GPU tests (test_gpu_transform.py) hold the device to is
only as good as this model."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import transform_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dsopp_hip_transformer_create", "dsopp_hip_transformer_destroy", "dsopp_hip_transformer_sizes", "dsopp_hip_transform_calibration",
               "dsopp_hip_transformer_transform_image", "dsopp_hip_transformer_transform_mask", "dsopp_hip_transformer_transform_device",
               "dsopp_hip_pyramid_build_transformed", "dsopp_hip_semantics_create_transformed")
ERR_INVALID_ARGUMENT, ERR_HIP = -1, -4
RATIOS = (0.3, 0.4, 0.5, 0.61, 0.75, 0.9, 0.91, 1.0, 1.5)


def _random(w, h, seed=0):
    return np.random.default_rng(seed + 1000 * w + h).integers(0, 256, (h, w)).astype(np.uint8)


@pytest.mark.parametrize("size", [(2, 2), (1, 1), (5, 3), (64, 48), (67, 45)], ids=lambda s: "%dx%d" % s)
def test_ratio_1_is_the_identity(size):
    src = _random(*size)
    assert np.array_equal(tm.resize_linear(src, size), src)
    assert np.array_equal(tm.resize_nearest(src, size), src)
    assert np.array_equal(tm.transform_image(src, 1.0, 0), src) and np.array_equal(tm.transform_mask(src, 1.0, 0), src)


@pytest.mark.parametrize("size", [(2, 2), (32, 32), (66, 46)], ids=lambda s: "%dx%d" % s)
def test_ratio_half_of_an_even_size_is_the_rounded_2x2_mean(size):
    src = _random(*size)
    p = src.astype(np.int64)
    mean = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2
    assert np.array_equal(tm.transform_image(src, 0.5, 0), mean.astype(np.uint8))


@pytest.mark.parametrize("ratio", [0.3, 0.4, 0.75, 1.5])
def test_a_constant_image_stays_constant(ratio):
    for value in (0, 1, 77, 128, 254, 255):
        out = tm.transform_image(np.full((45, 67), value, dtype=np.uint8), ratio, 0)
        assert out.shape == (int(45 * ratio), int(67 * ratio)) and (out == value).all(), (ratio, value)


def test_every_weight_pair_sums_to_2048_and_taps_stay_inside():
    for n_in in (2, 32, 45, 47, 50, 60, 65, 67, 70, 71, 80, 1024, 1280):
        for ratio in RATIOS:
            n_out = tm.resized_size(n_in, ratio)
            if n_out < 1:
                continue
            s0, s1, w0, w1 = tm.linear_axis(n_in, n_out)
            assert ((w0 + w1) == tm.COEF_ONE).all() and w0.min() >= 0 and w1.min() >= 0, (n_in, ratio)
            assert s0.min() >= 0 and s1.max() <= n_in - 1 and ((s1 == s0 + 1) | (w1 == 0)).all(), (n_in, ratio)
            assert (np.diff(s0) >= 0).all()
            near = tm.nearest_axis(n_in, n_out)
            assert near.min() >= 0 and near.max() <= n_in - 1 and (np.diff(near) >= 0).all()


@pytest.mark.parametrize("ratio", RATIOS)
def test_extreme_images_stay_within_a_byte(ratio):
    """0 / 255 noise: the largest steps the interpolation can meet (resize_linear itself asserts 0 .. 255 before it narrows)"""
    src = (np.random.default_rng(5).integers(0, 2, (50, 70)) * 255).astype(np.uint8)
    out = tm.transform_image(src, ratio, 0)
    assert out.dtype == np.uint8 and out.shape == (int(50 * ratio), int(70 * ratio))
    lo, hi = int(src.min()), int(src.max())
    assert out.min() >= lo and out.max() <= hi


def test_linear_between_its_two_taps_on_a_ramp():
    """a horizontal ramp resized to 1.5 times: every output lies between the two source pixels it interpolates.  The
    three truncating shifts lose less than 2 + 1/16 quarter grey levels before the rounding adds 2: at most one grey level below."""
    src = np.tile((np.arange(67) * 3).astype(np.uint8), (45, 1))
    out = tm.resize_linear(src, (100, 67)).astype(np.int64)
    s0, s1, _, _ = tm.linear_axis(67, 100)
    assert (out >= 3 * s0[None, :] - 1).all() and (out <= 3 * s1[None, :]).all()
    assert (out[:, -1] == 3 * 66).all() and (out[:, 0] == 0).all() and len(np.unique(out[0])) > 67


@pytest.mark.parametrize("ratio", RATIOS)
def test_nearest_contains_only_input_values(ratio):
    src = (np.random.default_rng(6).integers(0, 7, (45, 67)) * 37).astype(np.uint8)   # seven class codes
    out = tm.transform_mask(src, ratio, 0)
    assert out.shape == (int(45 * ratio), int(67 * ratio)) and set(np.unique(out)) <= set(np.unique(src))


def test_nearest_at_ratio_half_picks_the_even_pixels():
    src = _random(66, 46)
    assert np.array_equal(tm.transform_mask(src, 0.5, 0), src[0::2, 0::2])


def test_crop_is_the_top_left_slice():
    src = _random(70, 50)
    assert np.array_equal(tm.crop(src, 4), src[:48, :64]) and np.array_equal(tm.crop(src, 0), src)
    assert np.array_equal(tm.transform_image(src, 1.0, 4), src[:48, :64]) and np.array_equal(tm.transform_mask(src, 1.0, 4), src[:48, :64])
    whole = tm.resize_linear(_random(80, 60), (60, 45))
    assert np.array_equal(tm.transform_image(_random(80, 60), 0.75, 4), whole[:32, :48])


def test_sizes_of_the_shipped_configurations():
    """1280 x 1024 (tummono) at the ratios of mono / dense, standart, fast and extreme.yaml"""
    assert tm.sizes((1280, 1024), 1.0, 4) == ((1280, 1024), (1280, 1024))
    assert tm.sizes((1280, 1024), 0.75, 4) == ((960, 768), (960, 768))
    assert tm.sizes((1280, 1024), 0.5, 4) == ((640, 512), (640, 512))
    assert tm.sizes((1280, 1024), 0.4, 4) == ((512, 409), (512, 400))


# ---- through the C ABI, no device

def test_new_symbols_declared_and_exported():
    from dsopp_amd import capi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dsopp_hip.h")).read(), flags=re.S)
    lib = C.CDLL(capi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/dsopp_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in capi.SYMBOLS


K = (1043.5, 1047.25, 640.3, 511.9)


@pytest.mark.parametrize("ratio, levels, want_size, want_image_size", [
    (0.4, 4, (512, 400), (512.0, 400.0)),      # the image-size path 1024 * 0.4 = 409.6 -> 409 -> 400
    (0.75, 4, (960, 768), (960.0, 768.0)),
    (0.4, 0, (512, 409), (512.0, 409.0)),
    (1.0, 4, (1280, 1024), (1280.0, 1024.0)),
])
def test_calibration_matches_the_model(ratio, levels, want_size, want_image_size):
    from dsopp_amd import capi
    image_size, k, out_size = capi.transform_calibration((1280, 1024), ratio, levels, K)
    model_size, model_k = tm.transform_calibration((1280, 1024), K, ratio, levels)
    assert out_size == want_size == tm.sizes((1280, 1024), ratio, levels)[1]
    assert tuple(image_size) == want_image_size == tuple(model_size)
    assert np.array_equal(k, model_k) and np.array_equal(k, np.array(K) * ratio)   # no half-pixel shift of cx, cy
    # every output is optional
    size_only, none, _ = capi.transform_calibration((1280, 1024), ratio, levels)
    assert none is None and np.array_equal(size_only, image_size)


def test_calibration_of_an_odd_size_truncates_after_the_ratio():
    from dsopp_amd import capi
    image_size, _, out_size = capi.transform_calibration((71, 47), 0.9, 0, K)
    assert out_size == (63, 42) and tuple(image_size) == (63.0, 42.0)       # 63.9 and 42.3 before the size_t cast
    image_size, _, out_size = capi.transform_calibration((71, 47), 0.9, 4, K)
    assert out_size == (48, 32) and tuple(image_size) == (48.0, 32.0)


def _calibration_rc(in_w, in_h, ratio, levels):
    from dsopp_amd import capi
    size, k = np.zeros(2), np.zeros(4)
    w, h = C.c_int(), C.c_int()
    k_in = np.array(K)
    return capi.lib().dsopp_hip_transform_calibration(in_w, in_h, C.c_double(ratio), levels, k_in.ctypes.data_as(C.c_void_p),
                                                      size.ctypes.data_as(C.c_void_p), k.ctypes.data_as(C.c_void_p), C.byref(w), C.byref(h))


def _create_rc(in_w, in_h, ratio, levels):
    from dsopp_amd import capi
    h = C.c_void_p()
    rc = capi.lib().dsopp_hip_transformer_create(0, None, in_w, in_h, C.c_double(ratio), levels, C.byref(h))
    assert rc != 0 or h.value
    if h.value:
        capi.lib().dsopp_hip_transformer_destroy(h)
    return rc


BAD = [(64, 48, float("nan"), 4), (64, 48, float("inf"), 4), (64, 48, -float("inf"), 4), (64, 48, 0.0, 4), (64, 48, -0.5, 4),
       (0, 48, 1.0, 4), (64, 0, 1.0, 4), (-3, 48, 1.0, 0), (64, 48, 1.0, -1), (64, 48, 1.0, 9),
       (64, 15, 1.0, 4),            # the height crops to 0
       (64, 48, 0.3, 4),            # 19 x 14 crops to 16 x 0
       (64, 48, 0.01, 0),           # resizes to 0 x 0
       (65536, 32768, 1.0, 0),      # 2^31 pixels in
       (40000, 40000, 1.5, 0)]      # 3.6e9 pixels out


@pytest.mark.parametrize("in_w, in_h, ratio, levels", BAD)
def test_bad_arguments_are_refused_before_any_device_is_touched(in_w, in_h, ratio, levels):
    assert _calibration_rc(in_w, in_h, ratio, levels) == ERR_INVALID_ARGUMENT
    assert _create_rc(in_w, in_h, ratio, levels) == ERR_INVALID_ARGUMENT


def test_the_edges_of_the_argument_ranges_are_accepted():
    assert _calibration_rc(1, 1, 1.0, 0) == 0 and _calibration_rc(256, 256, 1.0, 8) == 0 and _calibration_rc(16, 16, 1.0, 4) == 0
    assert _calibration_rc(64, 48, 1e-300 * 1e300, 4) == 0


def test_no_cpu_fallback():
    """without a device the transformer cannot be created: DSOPP_HIP_ERR_HIP, never a host implementation"""
    from dsopp_amd import capi
    if capi.device_count() > 0:
        pytest.skip("a GPU is present")
    assert _create_rc(64, 48, 0.75, 4) == ERR_HIP
    assert _create_rc(64, 48, 1.0, 0) == ERR_HIP
    with pytest.raises(capi.HipError) as e:
        capi.Transformer((64, 48), 0.75)
    assert "-4" in str(e.value)
