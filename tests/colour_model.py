"""NumPy statement of the colour frame path (include/dsopp_hip.h, "Colour frames"): an 8-bit BGR image, interleaved, goes through the
remap and through the resize and crop channel by channel — the single-channel statements of undistort_model and transform_model, with
coordinates, reflection and weights shared between B, G and R — and is converted to grey last, in the 15-bit fixed point of an 8-bit
BGR2GRAY.  All in integers, so the device is held to it bit for bit.  Pinned by tests/test_colour.py."""
import numpy as np

import transform_model as tm
import undistort_model as um

GREY_B, GREY_G, GREY_R = 3735, 19235, 9798     # round(0.114, 0.587, 0.299 * 2^15), summing to 2^15
GREY_SHIFT = 15


def _check(bgr):
    bgr = np.asarray(bgr)
    assert bgr.dtype == np.uint8 and bgr.ndim == 3 and bgr.shape[2] == 3, (bgr.dtype, bgr.shape)
    return bgr


def bgr_to_grey(bgr):
    """(..., 3) uint8 BGR -> (...) uint8: (3735 B + 19235 G + 9798 R + 16384) >> 15"""
    c = np.asarray(bgr)
    assert c.dtype == np.uint8 and c.shape[-1] == 3, (c.dtype, c.shape)
    c = c.astype(np.int64)
    total = GREY_B * c[..., 0] + GREY_G * c[..., 1] + GREY_R * c[..., 2]
    return ((total + (1 << (GREY_SHIFT - 1))) >> GREY_SHIFT).astype(np.uint8)


def _per_channel(bgr, stage):
    return np.ascontiguousarray(np.stack([stage(np.ascontiguousarray(bgr[..., c])) for c in range(3)], axis=-1))


def remap_bgr(bgr, map_x, map_y):
    """cv::remap of a CV_8UC3 image: um.remap of every channel with the same maps"""
    return _per_channel(_check(bgr), lambda channel: um.remap(channel, map_x, map_y))


def transform_bgr(bgr, ratio, levels):
    """runImageTransformers of a CV_8UC3 image: tm.transform_image of every channel"""
    return _per_channel(_check(bgr), lambda channel: tm.transform_image(channel, ratio, levels))


def frame(bgr, maps, ratio, levels):
    """the camera's frame as CameraFeatures holds it: maps = (map_x, map_y) or None = no undistorter; ratio 1.0 and levels 0 = no
    transformer.  -> (colour (h, w, 3), grey (h, w)): image() and frameData()"""
    colour = _check(bgr)
    if maps is not None:
        colour = remap_bgr(colour, *maps)
    colour = transform_bgr(colour, ratio, levels)
    return colour, bgr_to_grey(colour)
