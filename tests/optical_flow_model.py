"""NumPy statement of the device optical-flow tracker's arithmetic (include/dsopp_hip.h, dsopp_hip_flow_tracker_create): the pyramidal
Lucas-Kanade tracker of features::OpticalFlowMatch (optical_flow.cpp:30-31), restated from OpenCV 4's calcOpticalFlowPyrLK (the scalar
path of lkpyramid.cpp) for 8-bit single-channel images.  Integers are int64, every float step is one np.float32 operation in the
written order, and the window sums are exact, so the device is held to it bit for bit.  Parity with OpenCV itself is not pinned (OpenCV
sums the window in float in raster order; the exact sum is the order-free statement of it).  Pinned by tests/test_optical_flow.py."""
import numpy as np

from undistort_model import reflect_101

F = np.float32
W_BITS = 14
ONE = 1 << W_BITS                 # 16384
SCALE = F(1.0 / (1 << 20))        # FLT_SCALE
FLT_EPSILON = F(np.finfo(np.float32).eps)


def descale(x, n):
    """(x + (1 << (n - 1))) >> n with an arithmetic shift"""
    return (np.asarray(x, dtype=np.int64) + (1 << (n - 1))) >> n


def pyr_down(src):
    """cv::pyrDown of an 8-bit image: the 1 4 6 4 1 taps on both axes, REFLECT_101, (sum + 128) >> 8; the size is ((w + 1) / 2, (h + 1) / 2)"""
    s = np.asarray(src).astype(np.int64)
    H, W = s.shape
    ow, oh = (W + 1) // 2, (H + 1) // 2
    x = 2 * np.arange(ow)
    col = [reflect_101(x + d, W) for d in (-2, -1, 0, 1, 2)]
    r = s[:, col[0]] + s[:, col[4]] + 4 * (s[:, col[1]] + s[:, col[3]]) + 6 * s[:, col[2]]
    y = 2 * np.arange(oh)
    row = [reflect_101(y + d, H) for d in (-2, -1, 0, 1, 2)]
    total = r[row[0]] + r[row[4]] + 4 * (r[row[1]] + r[row[3]]) + 6 * r[row[2]]
    return ((total + 128) >> 8).astype(np.uint8)


def scharr(src):
    """(H, W, 2) int16: the Scharr derivatives (dx, dy) of an 8-bit image, neighbours through REFLECT_101"""
    s = np.asarray(src).astype(np.int64)
    H, W = s.shape
    up, down = s[reflect_101(np.arange(H) - 1, H)], s[reflect_101(np.arange(H) + 1, H)]
    t0 = (up + down) * 3 + s * 10
    t1 = down - up
    left, right = reflect_101(np.arange(W) - 1, W), reflect_101(np.arange(W) + 1, W)
    dx = t0[:, right] - t0[:, left]
    dy = (t1[:, right] + t1[:, left]) * 3 + t1 * 10
    return np.stack([dx, dy], axis=-1).astype(np.int16)


def num_levels(width, height, window=15, max_level=3):
    """buildOpticalFlowPyramid's stop rule: after level l the size is halved; a halved width or height <= window ends the pyramid"""
    n, w, h = 1, width, height
    while n <= max_level:
        w, h = (w + 1) // 2, (h + 1) // 2
        if w <= window or h <= window:
            break
        n += 1
    return n


def build_levels(image, window=15, max_level=3):
    levels = [np.ascontiguousarray(image, dtype=np.uint8)]
    for _ in range(num_levels(image.shape[1], image.shape[0], window, max_level) - 1):
        levels.append(pyr_down(levels[-1]))
    return levels


def weights(a, b):
    """the four 14-bit bilinear weights of the f32 fractions (a, b); iw11 takes the remainder, so they sum to 16384"""
    a, b = F(a), F(b)
    iw00 = int(np.rint((F(1) - a) * (F(1) - b) * F(ONE)))
    iw01 = int(np.rint(a * (F(1) - b) * F(ONE)))
    iw10 = int(np.rint((F(1) - a) * b * F(ONE)))
    return iw00, iw01, iw10, ONE - iw00 - iw01 - iw10


def sample_image(img, ix, iy, win, w4, bits):
    """the window at integer origin (ix, iy) of an 8-bit plane read through REFLECT_101"""
    H, W = img.shape
    p = img.astype(np.int64)
    x0, x1 = reflect_101(ix + np.arange(win), W), reflect_101(ix + 1 + np.arange(win), W)
    y0, y1 = reflect_101(iy + np.arange(win), H)[:, None], reflect_101(iy + 1 + np.arange(win), H)[:, None]
    v = p[y0, x0] * w4[0] + p[y0, x1] * w4[1] + p[y1, x0] * w4[2] + p[y1, x1] * w4[3]
    return descale(v, bits)


def sample_deriv(plane, ix, iy, win, w4):
    """the same of one int16 derivative plane, which reads 0 outside the level"""
    H, W = plane.shape
    p = np.zeros((H + 2 * win + 2, W + 2 * win + 2), dtype=np.int64)
    p[win + 1:win + 1 + H, win + 1:win + 1 + W] = plane
    x = ix + win + 1 + np.arange(win)
    y = (iy + win + 1 + np.arange(win))[:, None]
    v = p[y, x] * w4[0] + p[y, x + 1] * w4[1] + p[y + 1, x] * w4[2] + p[y + 1, x + 1] * w4[3]
    return descale(v, W_BITS)


def _f32_sum(values):
    """the exact integer sum, rounded once to f32"""
    return F(int(np.sum(values, dtype=np.int64)))


def _floor(x):
    """floor as an integer; anything beyond +-1e9 and NaN become -1e9, which every range test refuses"""
    f = np.floor(x)
    return int(f) if -1e9 <= f <= 1e9 else -1000000000


def _outside(ix, iy, win, W, H):
    return ix < -win or ix >= W or iy < -win or iy >= H


class Tracker:
    """the reference image's levels and Scharr planes, kept across track() calls as the device object keeps them"""

    def __init__(self, width, height, window=15, max_level=3, max_iterations=10, epsilon=0.01, min_eig_threshold=1e-4):
        assert window % 2 == 1 and 3 <= window <= 15 and width >= 2 and height >= 2 and 0 <= max_level <= 5
        self.width, self.height, self.win, self.max_level = width, height, window, max_level
        self.max_count = min(max(int(max_iterations), 0), 100)
        eps = min(max(float(epsilon), 0.0), 10.0)
        self.eps2 = eps * eps                                  # f64
        self.min_eig = float(min_eig_threshold)
        self.n_levels = num_levels(width, height, window, max_level)
        self.reference = self.derivatives = self.target = None

    def set_reference(self, image):
        assert image.shape == (self.height, self.width)
        self.reference = build_levels(image, self.win, self.max_level)
        self.derivatives = [scharr(l) for l in self.reference]

    def track(self, image, points):
        """(points_to (n, 2) f32, status (n,) u8, err (n,) f32, iterations (n, n_levels) i32)"""
        assert self.reference is not None and image.shape == (self.height, self.width)
        self.target = build_levels(image, self.win, self.max_level)
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 2)
        n = len(pts)
        out, status = np.zeros((n, 2), np.float32), np.zeros(n, np.uint8)
        err, iters = np.zeros(n, np.float32), np.zeros((n, self.n_levels), np.int32)
        for i in range(n):
            out[i], status[i], err[i], iters[i] = self._track_point(pts[i])
        return out, status, err, iters

    def _track_point(self, pt):
        win = self.win
        half = F((win - 1) * 0.5)
        status, err = 1, F(0)
        iters = np.zeros(self.n_levels, np.int32)
        result = np.zeros(2, np.float32)
        for level in range(self.n_levels - 1, -1, -1):
            I_img, D, J_img = self.reference[level], self.derivatives[level], self.target[level]
            H, W = I_img.shape
            prev = pt * F(1.0 / (1 << level))
            nxt = prev.copy() if level == self.n_levels - 1 else result * F(2)
            result = nxt.copy()
            prev = prev - half
            ipx, ipy = _floor(prev[0]), _floor(prev[1])
            if _outside(ipx, ipy, win, W, H):
                if level == 0:
                    status, err = 0, F(0)
                continue
            w4 = weights(prev[0] - F(ipx), prev[1] - F(ipy))
            I = sample_image(I_img, ipx, ipy, win, w4, W_BITS - 5)
            Ix = sample_deriv(D[..., 0], ipx, ipy, win, w4)
            Iy = sample_deriv(D[..., 1], ipx, ipy, win, w4)
            A11, A12, A22 = _f32_sum(Ix * Ix) * SCALE, _f32_sum(Ix * Iy) * SCALE, _f32_sum(Iy * Iy) * SCALE
            det = A11 * A22 - A12 * A12
            min_eig = (A22 + A11 - np.sqrt((A11 - A22) * (A11 - A22) + F(4) * A12 * A12)) / F(2 * win * win)
            if float(min_eig) < self.min_eig or det < FLT_EPSILON:
                if level == 0:
                    status = 0
                continue
            det = F(1) / det
            nxt = nxt - half
            prev_delta = np.zeros(2, np.float32)
            for j in range(self.max_count):
                inx, iny = _floor(nxt[0]), _floor(nxt[1])
                if _outside(inx, iny, win, W, H):
                    if level == 0:
                        status = 0
                    break
                iters[level] = j + 1
                w4 = weights(nxt[0] - F(inx), nxt[1] - F(iny))
                diff = sample_image(J_img, inx, iny, win, w4, W_BITS - 5) - I
                b1, b2 = _f32_sum(diff * Ix) * SCALE, _f32_sum(diff * Iy) * SCALE
                delta = np.array([(A12 * b2 - A22 * b1) * det, (A12 * b1 - A11 * b2) * det], dtype=np.float32)
                nxt = nxt + delta
                result = nxt + half
                if float(delta[0]) * float(delta[0]) + float(delta[1]) * float(delta[1]) <= self.eps2:
                    break
                if j > 0 and abs(float(delta[0] + prev_delta[0])) < 0.01 and abs(float(delta[1] + prev_delta[1])) < 0.01:
                    result = result - delta * F(0.5)
                    break
                prev_delta = delta
            if level == 0 and status == 1:
                q = result - half
                iqx, iqy = _floor(q[0]), _floor(q[1])
                if _outside(iqx, iqy, win, W, H):
                    status = 0
                else:
                    w4 = weights(q[0] - F(iqx), q[1] - F(iqy))
                    diff = sample_image(J_img, iqx, iqy, win, w4, W_BITS - 5) - I
                    err = F(int(np.sum(np.abs(diff), dtype=np.int64))) / F(32 * win * win)
        return result, status, err, iters
