"""NumPy statement of the device ORB keypoint detector's arithmetic (include/dsopp_hip.h, dsopp_hip_orb_detector_create): the keypoint
positions of cv::ORB::create(nfeatures, 2.0f, 5) with HARRIS_SCORE — level images and masks, FAST-9/16 scores, 3 x 3 suppression, the
mask and border filters, retainBest(2 n_l) on the FAST score, the Harris response and retainBest(n_l) on it — and findCorrespondences
on top of it.  Integers throughout, and one float32 chain of single operations for the Harris response, so the device is held to it
bit for bit.  Written from the statement in the header, not from the kernels; pinned by tests/test_orb_detector.py."""
import numpy as np

from transform_model import resize_linear

F = np.float32
RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2),
        (-1, 3)]                                                   # (dx, dy), a closed walk round the centre
HARRIS_BLOCK = 7
HARRIS_K = F(0.04)


def cv_round(x):
    """to nearest, ties to even"""
    return int(np.rint(x))


def features_per_level(nfeatures, nlevels):
    """step 1: the features each level may return"""
    factor = F(0.5)
    nd = F(nfeatures) * (F(1) - factor) / (F(1) - F(np.power(np.float64(factor), np.float64(nlevels))))
    out = []
    for _ in range(nlevels - 1):
        out.append(cv_round(nd))
        nd = nd * factor
    out.append(max(nfeatures - sum(out), 0))
    return out


def level_size(width, height, level):
    return cv_round(width / 2.0 ** level), cv_round(height / 2.0 ** level)


def build_levels(image, nlevels):
    """step 2"""
    h, w = image.shape
    levels = [np.ascontiguousarray(image, dtype=np.uint8)]
    for l in range(1, nlevels):
        levels.append(resize_linear(levels[-1], level_size(w, h, l)))
    return levels


def build_mask_levels(mask, nlevels):
    """step 3: the bytes at level 0, above it the resize of the level below followed by threshold(254, THRESH_TOZERO)"""
    h, w = mask.shape
    levels = [np.ascontiguousarray(mask, dtype=np.uint8)]
    for l in range(1, nlevels):
        m = resize_linear(levels[-1], level_size(w, h, l))
        levels.append(np.where(m > 254, m, 0).astype(np.uint8))
    return levels


def fast_arc_measure(image):
    """step 4's m for every centre 3 <= x < w - 3, 3 <= y < h - 3 as an (h - 6, w - 6) array (None when there is no centre)"""
    h, w = image.shape
    if w < 7 or h < 7:
        return None
    p = image.astype(np.int32)
    v = p[3:h - 3, 3:w - 3]
    d = [p[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] - v for dx, dy in RING]
    m = None
    for sign in (1, -1):
        for start in range(16):
            arc = sign * d[start]
            for k in range(1, 9):
                arc = np.minimum(arc, sign * d[(start + k) % 16])
            m = arc if m is None else np.maximum(m, arc)
    return m


def fast_scores(image, threshold):
    """step 4: the score plane, one byte per pixel; 0 where there is no corner"""
    h, w = image.shape
    out = np.zeros((h, w), np.uint8)
    m = fast_arc_measure(image)
    if m is not None:
        out[3:h - 3, 3:w - 3] = np.where(m > threshold, m - 1, 0)
    return out


def suppress(scores):
    """step 5: True where the score is strictly greater than the scores of the 8 neighbours"""
    h, w = scores.shape
    s = np.zeros((h + 2, w + 2), np.int32)
    s[1:-1, 1:-1] = scores
    around = np.zeros((h, w), np.int32)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                around = np.maximum(around, s[1 + dy:1 + dy + h, 1 + dx:1 + dx + w])
    return s[1:-1, 1:-1] > around


def filter_survivors(survivors, mask, edge):
    """step 6: (x, y) of the survivors off masked pixels and inside the border, in raster order"""
    h, w = survivors.shape
    keep = survivors.copy()
    if mask is not None:
        keep &= mask != 0
    inside = np.zeros((h, w), bool)
    if w > 2 * edge and h > 2 * edge:
        inside[edge:h - edge, edge:w - edge] = True
    ys, xs = np.nonzero(keep & inside)              # np.nonzero walks rows, then columns: ascending y, then x
    return xs, ys


def retain_best(values, n):
    """steps 7 and 9, KeyPointsFilter::retainBest: the indices that stay, ascending"""
    values = np.asarray(values)
    if len(values) <= n:
        return np.arange(len(values))
    if n == 0:
        return np.arange(0)
    least = np.sort(values)[::-1][n - 1]
    return np.nonzero(values >= least)[0]


def harris_sums(image, x, y):
    """step 8's integer sums a, b, c"""
    p = image[y - 4:y + 5, x - 4:x + 5].astype(np.int64)
    assert p.shape == (9, 9)
    c = slice(1, 8)
    ix = 2 * (p[c, 2:9] - p[c, 0:7]) + (p[0:7, 2:9] - p[0:7, 0:7]) + (p[2:9, 2:9] - p[2:9, 0:7])
    iy = 2 * (p[2:9, c] - p[0:7, c]) + (p[2:9, 0:7] - p[0:7, 0:7]) + (p[2:9, 2:9] - p[0:7, 2:9])
    return int((ix * ix).sum()), int((iy * iy).sum()), int((ix * iy).sum())


def harris_scale4():
    scale = F(1) / (F(4 * HARRIS_BLOCK) * F(255))
    return scale * scale * scale * scale


def harris_from_sums(a, b, c):
    fa, fb, fc = F(a), F(b), F(c)
    return ((fa * fb - fc * fc) - (HARRIS_K * (fa + fb)) * (fa + fb)) * harris_scale4()


def harris_response(image, x, y):
    return harris_from_sums(*harris_sums(image, x, y))


class Detection:
    """everything a detect leaves: the planes per level, the lists after each step per level, and the output"""

    def __init__(self):
        self.images, self.masks, self.scores = [], None, []
        self.filtered, self.first_cut, self.final = [], [], []     # per level: (xs, ys) / (xs, ys, fast) / (xs, ys, response)
        self.xy = self.level = self.response = None


def detect(image, mask=None, nfeatures=500, nlevels=5, edge_threshold=31, fast_threshold=20):
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim == 2
    out = Detection()
    out.images = build_levels(image, nlevels)
    out.masks = None if mask is None else build_mask_levels(np.asarray(mask), nlevels)
    per_level = features_per_level(nfeatures, nlevels)
    xy, level, response = [], [], []
    for l in range(nlevels):
        img = out.images[l]
        scores = fast_scores(img, fast_threshold)
        out.scores.append(scores)
        xs, ys = filter_survivors(suppress(scores), None if out.masks is None else out.masks[l], edge_threshold)
        out.filtered.append((xs, ys))
        fast = scores[ys, xs].astype(np.int64)
        keep = retain_best(fast, 2 * per_level[l])
        xs, ys, fast = xs[keep], ys[keep], fast[keep]
        out.first_cut.append((xs, ys, fast))
        r = np.array([harris_response(img, int(x), int(y)) for x, y in zip(xs, ys)], dtype=np.float32)
        keep = retain_best(r, per_level[l])
        xs, ys, r = xs[keep], ys[keep], r[keep]
        out.final.append((xs, ys, r))
        up = F(1 << l)
        xy.append(np.stack([xs.astype(np.float32) * up, ys.astype(np.float32) * up], axis=1).reshape(-1, 2))
        level.append(np.full(len(xs), l, np.int32))
        response.append(r)
    out.xy = np.concatenate(xy).astype(np.float32).reshape(-1, 2)
    out.level = np.concatenate(level).astype(np.int32)
    out.response = np.concatenate(response).astype(np.float32)
    return out


def find_correspondences(features_from, tracker, image_to, detection_xy, nfeatures, shuffle_order):
    """features::findCorrespondences over the flow finder.  features_from None: the detection, no correspondences.  Else `tracker` (an
    optical_flow_model.Tracker whose reference is image_from) tracks features_from into image_to: a feature and a correspondence
    (idx_from, idx_to) per status != 0, then new[order[i]] is appended while fewer than nfeatures are held; order =
    shuffle_order(len(detection_xy)).  -> (features (n, 2) float32, correspondences (m, 2) int64)"""
    new = np.asarray(detection_xy, np.float32).reshape(-1, 2)
    if features_from is None:
        return new.copy(), np.zeros((0, 2), np.int64)
    to, status, _, _ = tracker.track(image_to, features_from)
    features, correspondences = [], []
    for i in range(len(status)):
        if status[i] != 0:
            features.append(to[i])
            correspondences.append((i, len(features) - 1))
    order = shuffle_order(len(new))
    i = 0
    while len(features) < nfeatures and i < len(order):
        features.append(new[order[i]])
        i += 1
    return np.array(features, np.float32).reshape(-1, 2), np.array(correspondences, np.int64).reshape(-1, 2)
