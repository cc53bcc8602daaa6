"""The NumPy model of the colour frame path (tests/colour_model.py) against closed forms.  What the GPU tests (test_gpu_colour.py) hold
the device to is only as good as this model.  The last test says what the path is for: converting to grey behind the stages, as the
reference does, is not converting in front of them."""
import numpy as np

import colour_model as cm
import transform_model as tm
import undistort_model as um


def _random_bgr(w, h, seed=0):
    return np.random.default_rng(seed + 1000 * w + h).integers(0, 256, (h, w, 3)).astype(np.uint8)


def _half_pixel_maps(w, h):
    mx, my = um.identity_maps(w, h)
    return mx + np.float32(0.5), my + np.float32(0.5)


def test_every_grey_maps_to_itself():
    v = np.arange(256, dtype=np.uint8)
    assert np.array_equal(cm.bgr_to_grey(np.stack([v, v, v], axis=-1)), v)
    assert cm.GREY_B + cm.GREY_G + cm.GREY_R == 1 << cm.GREY_SHIFT


def test_the_pure_primaries():
    primaries = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255]], dtype=np.uint8)     # blue, green, red
    got = cm.bgr_to_grey(primaries)
    assert got.tolist() == [29, 150, 76] and int(got.sum()) == 255


def test_the_fixed_point_is_within_0_505_of_the_float_formula():
    """coefficient rounding: at most 255 * 0.552 / 32768 = 0.0043; the final rounding: 0.5"""
    bgr = np.random.default_rng(5).integers(0, 256, (200_000, 3)).astype(np.uint8)
    exact = 0.114 * bgr[:, 0] + 0.587 * bgr[:, 1] + 0.299 * bgr[:, 2]
    worst = np.abs(cm.bgr_to_grey(bgr).astype(np.float64) - exact).max()
    print("largest distance from the float formula:", worst)
    assert worst <= 0.505


def test_the_stages_are_the_single_channel_models_channel_by_channel():
    bgr = _random_bgr(80, 60)
    maps = _half_pixel_maps(80, 60)
    remapped, transformed = cm.remap_bgr(bgr, *maps), cm.transform_bgr(bgr, 0.75, 4)
    assert remapped.shape == (60, 80, 3) and transformed.shape == (32, 48, 3)
    for c in range(3):
        channel = np.ascontiguousarray(bgr[..., c])
        assert np.array_equal(remapped[..., c], um.remap(channel, *maps))
        assert np.array_equal(transformed[..., c], tm.transform_image(channel, 0.75, 4))
    assert not np.array_equal(remapped[..., 0], remapped[..., 1])
    colour, grey = cm.frame(bgr, maps, 0.75, 4)
    assert np.array_equal(colour, cm.transform_bgr(remapped, 0.75, 4)) and np.array_equal(grey, cm.bgr_to_grey(colour))
    colour, grey = cm.frame(bgr, None, 1.0, 0)
    assert np.array_equal(colour, bgr) and np.array_equal(grey, cm.bgr_to_grey(bgr))


def test_a_grey_frame_in_three_channels_gives_the_grey_path():
    v = _random_bgr(80, 60)[..., 0]
    colour, grey = cm.frame(np.stack([v, v, v], axis=-1), _half_pixel_maps(80, 60), 0.75, 4)
    assert np.array_equal(grey, tm.transform_image(um.remap(v, *_half_pixel_maps(80, 60)), 0.75, 4))
    assert all(np.array_equal(colour[..., c], grey) for c in range(3))


def test_grey_last_is_not_grey_first():
    """the reference converts behind the stages (camera_features.cpp:32), a grey-only library in front of them: the two orders differ
    by the rounding of the conversion — in many bytes, by one grey level each"""
    bgr = _random_bgr(80, 60)
    first = cm.bgr_to_grey(bgr)
    for name, last, grey_first in (
            ("resize 0.75, crop 4", cm.frame(bgr, None, 0.75, 4)[1], tm.transform_image(first, 0.75, 4)),
            ("half-pixel remap", cm.frame(bgr, _half_pixel_maps(80, 60), 1.0, 0)[1], um.remap(first, *_half_pixel_maps(80, 60)))):
        difference = np.abs(last.astype(np.int64) - grey_first.astype(np.int64))
        print(f"{name}: {int((difference != 0).sum())} of {difference.size} grey bytes differ, by at most {int(difference.max())}")
        assert last.shape == grey_first.shape
        assert (difference != 0).any() and difference.max() <= 1
