"""NumPy statement of the remap tables the device builds from a camera model (include/dsopp_hip.h, dsopp_hip_undistorter_create_from_model):
the pinhole unprojection of every output pixel, the projection of its ray through the simple-radial, TUM-FOV or atan model, the float
map entry, and the simple-radial constructor's constants (numpy.roots where the library has its own root finder).  Everything is
binary64 in the stated order; NumPy never fuses a product and a sum.  A camera is a tuple (type, parameters...) as CAMERAS builds them.
Pinned by tests/test_camera_remap.py; tests/test_gpu_camera_remap.py holds the device to it."""
import functools

import numpy as np

BORDER = 4                   # CameraModelBase::kBorderSize (camera_model_base.hpp:34)
SIMPLE_RADIAL, TUM_FOV, ATAN = "simple_radial", "tum_fov", "atan"
ATAN_POLYNOMIAL = (0.0, 0.0591006, 0.0, -0.0105943, 0.0, -0.00467958, 0.0, 0.000500274)   # the reference test's (undistorter.cpp:71)

# the GPU tests' cameras, scaled with the size
CAMERAS = {
    "sr_mild": lambda w, h: (SIMPLE_RADIAL, 0.8 * w, 0.49 * w, 0.51 * h, -0.25, 0.06),
    "sr_leaves_roi": lambda w, h: (SIMPLE_RADIAL, 0.8 * w, 0.49 * w, 0.51 * h, 0.4, 0.05),
    "sr_radius": lambda w, h: (SIMPLE_RADIAL, 0.5 * w, 0.5 * w, 0.5 * h, -0.6, 0.05),
    "sr_zero": lambda w, h: (SIMPLE_RADIAL, 0.5 * w, 0.5 * w, 0.5 * h, 0.0, 0.0),
    "fov": lambda w, h: (TUM_FOV, 0.7 * w, 0.72 * h, 0.51 * w, 0.48 * h, 0.93),
    "fov_off_centre": lambda w, h: (TUM_FOV, 0.7 * w, 0.72 * h, 0.62 * w, 0.40 * h, 0.93),
    "atan_poly": lambda w, h: (ATAN, 0.28 * w, 0.28 * w, 0.47 * w, 0.49 * h) + ATAN_POLYNOMIAL,
    "atan_plain": lambda w, h: (ATAN, 0.28 * w, 0.28 * w, 0.47 * w, 0.49 * h),
}


def inside_roi(x, y, width, height):
    """CameraModelBase::insideCameraROI (camera_model_base.hpp:52-60); false for NaN"""
    with np.errstate(invalid="ignore"):
        return (x >= BORDER) & (y >= BORDER) & (x <= width - BORDER - 1) & (y <= height - BORDER - 1)


def focals(camera):
    return (camera[1], camera[1]) if camera[0] == SIMPLE_RADIAL else (camera[1], camera[2])


def pinhole_intrinsics(width, height, camera):
    """the target of constructRemaps (undistorter.hpp:70-80)"""
    fx, fy = focals(camera)
    return np.array([fx, fy, width / 2.0, height / 2.0])


def pinhole_rays(width, height, fx, fy):
    """PinholeCamera::unproject at every pixel (pinhole_camera.hpp:129-141): a product with the inverse focal length"""
    x, y = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    return (x - width / 2.0) * (1.0 / fx), (y - height / 2.0) * (1.0 / fy), inside_roi(x, y, width, height)


# ---- the simple-radial constructor (simple_radial.hpp:47-82)

def minimal_positive_root(polynomial):
    """polynomial_solver.hpp:11-41 with numpy.roots for the companion matrix's eigenvalues; coefficients from the constant upwards"""
    c = np.asarray(polynomial, dtype=np.float64)
    c = c / np.sqrt(np.sum(c * c))
    n = len(c) - 1
    while abs(c[n]) < 1e-8:
        n -= 1
    if n == 0:
        return 0.0
    roots = np.roots(c[:n + 1][::-1])
    answer = np.inf
    for l in roots:
        if abs(l.imag) > np.finfo(np.float64).eps * abs(l.real) or l.real < 0.0:
            continue
        answer = min(answer, float(l.real))
    return answer


def simple_radial_derived(width, height, f, cx, cy, k1, k2):
    """(max_valid_radius_, line_after_radius_(0), line_after_radius_(1)) and whether the extremum rule replaced the root"""
    f, cx, cy, k1, k2 = (np.float64(v) for v in (f, cx, cy, k1, k2))
    max_x, max_y = max(cx, width - cx), max(cy, height - cy)
    radius = np.float64(minimal_positive_root([-(np.sqrt(max_x * max_x + max_y * max_y) / f), 1.0, 0.0, k1, 0.0, k2]))
    replaced = False
    discriminant = 9.0 * k1 * k1 - 20.0 * k2
    with np.errstate(all="ignore"):   # k2 == 0: the divisions give NaN or inf, as in the reference
        if discriminant >= 0.0:
            root1_2 = (-3.0 * k1 - np.sqrt(discriminant)) / 10.0 / k2
            root2_2 = (-3.0 * k1 + np.sqrt(discriminant)) / 10.0 / k2
            root = radius
            if root1_2 > 0.0:
                root = np.sqrt(root1_2)
            elif root2_2 > 0.0:
                root = np.sqrt(root2_2)
            if root < radius:
                radius, replaced = root - BORDER / f, True
        r2 = radius * radius
        r4 = r2 * r2
        line1 = radius * (1.0 + k1 * r2 + k2 * r4)
        line0 = 1.0 + 3.0 * k1 * r2 + 5.0 * k2 * r4
    return np.array([radius, line0, line1]), replaced


# ---- the projections: (px, py, success, reason of the failure)

RADIUS, ROI = 1, 2   # failure reasons beyond the pinhole's border (0 = none)


def project(width, height, camera, rx, ry, max_valid_radius=None):
    """the distorted model's projection of the rays (rx, ry, 1): points in binary64, success flags, the failing branch"""
    kind = camera[0]
    with np.errstate(all="ignore"):
        if kind == SIMPLE_RADIAL:
            _, f, cx, cy, k1, k2 = camera
            if max_valid_radius is None:
                max_valid_radius = simple_radial_derived(width, height, f, cx, cy, k1, k2)[0][0]
            r2 = rx * rx + ry * ry
            beyond = np.sqrt(r2) > max_valid_radius
            d = (1.0 + k1 * r2) + (k2 * r2) * r2
            px, py = (rx * d) * f + cx, (ry * d) * f + cy
            roi = inside_roi(px, py, width, height)
            return px, py, ~beyond & roi, np.where(beyond, RADIUS, np.where(roi, 0, ROI))
        if kind == TUM_FOV:
            _, fx, fy, cx, cy, fov = camera
            ru = np.sqrt(rx * rx + ry * ry)
            centre = ru < 1e-8
            rd = np.arctan2((2.0 * ru) * np.tan(fov / 2.0), 1.0) / fov
            q = rd / np.where(centre, 1.0, ru)
            px, py = np.where(centre, cx, (q * rx) * fx + cx), np.where(centre, cy, (q * ry) * fy + cy)
        else:
            fx, fy, cx, cy = camera[1:5]
            k = camera[5:]
            n = np.sqrt((rx * rx + ry * ry) + 1.0)
            ax, ay, az = rx / n, ry / n, 1.0 / n
            rho = np.sqrt(ax * ax + ay * ay)
            centre = rho < 1e-6
            theta = np.arctan2(rho, az)
            s = np.zeros_like(theta)
            for coefficient in k[::-1]:
                s = s * theta + coefficient
            s = theta * (1.0 + s * theta)
            safe = np.where(centre, 1.0, rho)
            px, py = np.where(centre, cx, ((ax * s) / safe) * fx + cx), np.where(centre, cy, ((ay * s) / safe) * fy + cy)
        roi = centre | inside_roi(px, py, width, height)
        return px, py, roi, np.where(roi, 0, ROI)


class Tables:
    """everything the tests ask of one (size, camera): points in binary64, flags, the float maps"""

    def __init__(self, width, height, camera, max_valid_radius=None):
        fx, fy = focals(camera)
        self.rx, self.ry, self.in_border = pinhole_rays(width, height, fx, fy)
        self.px, self.py, projected, reason = project(width, height, camera, self.rx, self.ry, max_valid_radius)
        self.ok = self.in_border & projected
        self.reason = np.where(self.in_border, reason, 0)   # which projection branch failed, among the pixels the pinhole accepts
        self.map_x = np.where(self.ok, self.px, -1.0).astype(np.float32)   # round to nearest even
        self.map_y = np.where(self.ok, self.py, -1.0).astype(np.float32)
        for a in (self.rx, self.ry, self.px, self.py, self.ok, self.reason, self.map_x, self.map_y):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def tables(width, height, camera, max_valid_radius=None):
    return Tables(width, height, camera, max_valid_radius)


# ---- how close a binary64 value lies to a point where its float32 rounding flips

def spacings_to_midpoint(value):
    """the distance of each binary64 value from the nearest midpoint of two neighbouring float32 numbers, in spacings of the value"""
    v = np.asarray(value, dtype=np.float64)
    f = v.astype(np.float32)
    up = (f.astype(np.float64) + np.nextafter(f, np.float32(np.inf)).astype(np.float64)) / 2.0
    down = (f.astype(np.float64) + np.nextafter(f, np.float32(-np.inf)).astype(np.float64)) / 2.0
    return np.minimum(np.abs(v - up), np.abs(v - down)) / np.spacing(np.abs(v))


def spacings_to_roi_bound(tab, width, height):
    """the distance in pixels of each projected point from the nearest of the four ROI bounds"""
    with np.errstate(invalid="ignore"):
        return np.minimum.reduce([np.abs(tab.px - BORDER), np.abs(tab.py - BORDER), np.abs(tab.px - (width - BORDER - 1)),
                                  np.abs(tab.py - (height - BORDER - 1))])


# ---- the inverse: a projected point back to its pinhole ray

def radial_function(camera, r, max_valid_radius=None):
    """the distorted radius (in focal lengths) of a ray at pinhole radius r: monotone where the projection succeeds"""
    kind = camera[0]
    if kind == SIMPLE_RADIAL:
        k1, k2 = camera[4:6]
        r2 = r * r
        return r * ((1.0 + k1 * r2) + (k2 * r2) * r2)
    if kind == TUM_FOV:
        fov = camera[5]
        return np.arctan2(2.0 * r * np.tan(fov / 2.0), 1.0) / fov
    theta = np.arctan(r)
    s = np.zeros_like(theta)
    for coefficient in camera[5:][::-1]:
        s = s * theta + coefficient
    return theta * (1.0 + s * theta)


def unproject(camera, px, py, r_max):
    """the ray (rx, ry) at z = 1 whose projection is (px, py): bisection on radial_function over [0, r_max]"""
    if camera[0] == SIMPLE_RADIAL:
        fx = fy = camera[1]
        cx, cy = camera[2:4]
    else:
        fx, fy, cx, cy = camera[1:5]
    u, v = (px - cx) / fx, (py - cy) / fy
    target = np.hypot(u, v)
    lo, hi = np.zeros_like(target), np.full_like(target, r_max)
    for _ in range(100):
        mid = 0.5 * (lo + hi)
        below = radial_function(camera, mid) < target
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    r = 0.5 * (lo + hi)
    scale = np.where(target > 0, r / np.where(target > 0, target, 1.0), 0.0)
    return u * scale, v * scale


# ---- the reference's "three points on a line" (test/test/sensors/camera/calibration/undistorter.cpp:91-138)

def draw_discs(width, height, centres, radius=4):
    """cv::circle(img, centre, radius, 255, filled) for integer centres: the pixels within the radius"""
    img = np.zeros((height, width), dtype=np.uint8)
    y, x = np.mgrid[0:height, 0:width]
    for cx, cy in centres:
        img[(x - cx) ** 2 + (y - cy) ** 2 <= radius * radius] = 255
    return img
