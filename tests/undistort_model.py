"""NumPy statement of the device undistorter's arithmetic (include/dsopp_hip.h, dsopp_hip_undistorter_create): the fixed-point
bilinear remap of an 8-bit single-channel image with BORDER_REFLECT_101, all in integers, so the device is held to it bit for bit.
Also the remap tables of the reference's two distorted camera models, built as Undistorter::estimateRemaps builds them
(undistorter.hpp:124-142), for the GPU tests.  Pinned by tests/test_undistort.py."""
import numpy as np

FRACTION_BITS = 5            # 1 / 32 pixel
ONE = 1 << FRACTION_BITS
BORDER = 4                   # CameraModelBase::kBorderSize (camera_model_base.hpp:34)


def fixed_point(coordinate):
    """float32 coordinates -> (integer part = the floor, 5-bit fraction): rint(c * 32) with ties to even, split by an arithmetic shift"""
    c = np.asarray(coordinate, dtype=np.float32)
    s = np.rint(c * np.float32(32.0)).astype(np.int64)   # the product is exact in float32; np.rint rounds half to even
    return s >> FRACTION_BITS, s & (ONE - 1)


def reflect_101(index, n):
    """BORDER_REFLECT_101 of any integer for an axis of n >= 2 pixels: period 2 (n - 1), ... c b | a b c d | c b ..."""
    period = 2 * (n - 1)
    r = np.mod(np.asarray(index, dtype=np.int64), period)   # np.mod of a negative number is non-negative
    return np.where(r >= n, period - r, r)


def remap(src, map_x, map_y):
    """out[v, u] = the remap of src (H x W uint8) at (map_x[v, u], map_y[v, u]); maps float32 of the output's shape"""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 2 and min(src.shape) >= 2
    H, W = src.shape
    ix, fx = fixed_point(map_x)
    iy, fy = fixed_point(map_y)
    x0, x1 = reflect_101(ix, W), reflect_101(ix + 1, W)
    y0, y1 = reflect_101(iy, H), reflect_101(iy + 1, H)
    p = src.astype(np.int64)
    total = ((ONE - fx) * (ONE - fy) * ONE * p[y0, x0] + fx * (ONE - fy) * ONE * p[y0, x1] +
             (ONE - fx) * fy * ONE * p[y1, x0] + fx * fy * ONE * p[y1, x1])
    return ((total + 16384) >> 15).astype(np.uint8)


def identity_maps(width, height):
    x, y = np.meshgrid(np.arange(width, dtype=np.float32), np.arange(height, dtype=np.float32))
    return x, y


def _inside_roi(x, y, width, height):
    """CameraModelBase::insideCameraROI (camera_model_base.hpp:52-60)"""
    return (x >= BORDER) & (y >= BORDER) & (x <= width - BORDER - 1) & (y <= height - BORDER - 1)


def _pinhole_rays(width, height, fx, fy):
    """the target pinhole of constructRemaps (undistorter.hpp:70-80: the model's focal lengths, centre = size / 2) unprojected at
    every pixel (pinhole_camera.hpp:129-141): (ray x, ray y) at z = 1 and the success flag"""
    x, y = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    return (x - width / 2.0) / fx, (y - height / 2.0) / fy, _inside_roi(x, y, width, height)


def _as_maps(px, py, ok):
    """estimateRemaps (undistorter.hpp:134-140): the projected point as float, (-1, -1) where either step failed"""
    return np.where(ok, px, -1.0).astype(np.float32), np.where(ok, py, -1.0).astype(np.float32)


def simple_radial_max_radius(width, height, f, cx, cy, k1, k2):
    """SimpleRadialCamera's max_valid_radius_ (simple_radial.hpp:47-77): the least positive root of r + k1 r^3 + k2 r^5 = the corner
    radius, pulled inside the first extremum of that polynomial when there is one"""
    corner = np.hypot(max(cx, width - cx), max(cy, height - cy)) / f
    roots = np.roots([k2, 0.0, k1, 0.0, 1.0, -corner])
    real = roots[np.abs(roots.imag) < 1e-9].real
    radius = real[real > 0].min()
    disc = 9.0 * k1 * k1 - 20.0 * k2
    if disc >= 0:
        r1, r2 = (-3.0 * k1 - np.sqrt(disc)) / 10.0 / k2, (-3.0 * k1 + np.sqrt(disc)) / 10.0 / k2
        root = np.sqrt(r1) if r1 > 0 else (np.sqrt(r2) if r2 > 0 else radius)
        if root < radius:
            radius = root - BORDER / f
    return radius


def simple_radial_maps(width, height, f, cx, cy, k1, k2):
    """SimpleRadialCamera::project (simple_radial.hpp:134-160) of the pinhole's rays"""
    rx, ry, ok = _pinhole_rays(width, height, f, f)
    r2 = rx * rx + ry * ry
    ok = ok & ~(np.sqrt(r2) > simple_radial_max_radius(width, height, f, cx, cy, k1, k2))
    scale = 1.0 + k1 * r2 + k2 * r2 * r2
    px, py = rx * scale * f + cx, ry * scale * f + cy
    return _as_maps(px, py, ok & _inside_roi(px, py, width, height))


def tum_fov_maps(width, height, fx, fy, cx, cy, fov):
    """TUMFovModel::project (tum_fov_model.hpp:72-82) of the pinhole's rays"""
    rx, ry, ok = _pinhole_rays(width, height, fx, fy)
    r_u = np.hypot(rx, ry)
    small = r_u < 1e-8
    r_d = np.arctan2(2.0 * r_u * np.tan(fov / 2.0), 1.0) / fov
    ratio = np.where(small, 0.0, r_d / np.where(small, 1.0, r_u))
    px, py = np.where(small, cx, ratio * rx * fx + cx), np.where(small, cy, ratio * ry * fy + cy)
    return _as_maps(px, py, ok & (small | _inside_roi(px, py, width, height)))
