"""TEST INFRASTRUCTURE ONLY.  NumPy statement of what the library does with semantic segmentation, written from the reference's
definitions and independent of the device code:

  filter_mask            CameraMask::filterSemanticObjects      src/sensors/camera_calibration/src/camera_mask.cpp:31-39
  mask_level / pyramid   CameraMask::resize(1 / 2^l) of the finest mask, every level from level 0
                                                                 src/features/src/camera_features.cpp:71-84
  add_observations       addSemanticObservations                src/tracker/tracker/src/monocular_tracker.cpp:263-305
  semantic_type          ActiveTrackingLandmark::semanticTypeId src/track/landmarks/src/active_tracking_landmark.cpp:71-88

The reprojection is oracle/spec.py's project_pattern / in_roi."""
import numpy as np

from oracle import spec

STATUS_OK = 0


def filter_mask(static, cls, is_filtered):
    """level-0 mask bytes: a pixel of a filtered class leaves the static mask; without a filter or a class image the static mask"""
    static = np.asarray(static, dtype=np.uint8)
    if cls is None or is_filtered is None:
        return static.copy()
    return np.where(np.asarray(is_filtered, dtype=np.uint8)[np.asarray(cls, dtype=np.uint8)] != 0, 0, static).astype(np.uint8)


def mask_level(m0, level):
    """cv::resize(m0, INTER_LINEAR) to the ratio 2^-level: the sample point lies midway between the two centre pixels of each axis, the
    two weights are equal, so the value is the rounded mean of a 2 x 2 block of LEVEL 0 (not of the level below)"""
    if level == 0:
        return np.asarray(m0, dtype=np.uint8).copy()
    H, W = m0.shape
    s = 1 << level
    assert H % s == 0 and W % s == 0, (W, H, level)
    cy = s * np.arange(H // s) + s // 2 - 1
    cx = s * np.arange(W // s) + s // 2 - 1
    m = m0.astype(np.int64)
    total = m[np.ix_(cy, cx)] + m[np.ix_(cy, cx + 1)] + m[np.ix_(cy + 1, cx)] + m[np.ix_(cy + 1, cx + 1)]
    return ((total + 2) >> 2).astype(np.uint8)


def mask_pyramid(static, cls, is_filtered, levels):
    """validity (1 / 0) of every level's texels, and the level-0 mask bytes"""
    m0 = filter_mask(static, cls, is_filtered)
    return [(mask_level(m0, l) != 0).astype(np.uint8) for l in range(levels)], m0


def add_observations(frames, statuses, listed, hist=None, tie_eps=1e-9):
    """One addSemanticObservations(track, listed, model).
    frames: {id: dict(T = 4 x 4 T_world_agent, intr = (fx, fy, cx, cy), width, height, uv n x 2, idepth n, cls H x W uint8 or None,
    marginalized bool)}; statuses[(reference id, target id)] = connection statuses of the reference's landmarks.
    Returns (hist, pairs, near): hist[id] n x 256 uint8 (a copy of `hist` counted on, wrapping modulo 256), pairs[id][i] = the
    (landmark, target) pairs with status kOk that were reprojected for landmark i, near[id][i] = how many of them have a
    coordinate within tie_eps of an integer or of a ROI bound (where the last bit of another arithmetic could decide)."""
    out = {k: (np.zeros((len(f["uv"]), 256), dtype=np.uint8) if hist is None else hist[k].copy()) for k, f in frames.items()}
    pairs = {k: np.zeros(len(f["uv"]), dtype=np.int64) for k, f in frames.items()}
    near = {k: np.zeros(len(f["uv"]), dtype=np.int64) for k, f in frames.items()}
    listed = set(listed)

    def one_direction(r, t):
        fr, ft = frames[r], frames[t]
        if ft["cls"] is None:
            return
        st = statuses.get((r, t))
        if st is None:
            return
        T_tr = np.linalg.inv(ft["T"]) @ fr["T"]
        for i in range(len(st)):
            if st[i] != STATUS_OK:
                continue
            uv, d = fr["uv"][i], fr["idepth"][i]
            pts, z = spec.project_pattern(fr["intr"], ft["intr"], T_tr, uv, d)
            pairs[r][i] += 1
            bounds = np.concatenate([np.abs(pts[:, 0] - 4), np.abs(pts[:, 1] - 4), np.abs(pts[:, 0] - (ft["width"] - 5)), np.abs(pts[:, 1] - (ft["height"] - 5)),
                                     np.abs(pts - np.rint(pts)).ravel(), np.abs(z)])
            if np.any(bounds <= tie_eps) or not np.all(np.isfinite(pts)):
                near[r][i] += 1
            ok = (-1e-4 < d < 1010.0) and spec.in_roi(uv[None, :] + spec.PATTERN, fr["width"], fr["height"]) and bool(np.all(z > 0)) and \
                spec.in_roi(pts, ft["width"], ft["height"])
            if not ok:
                continue
            for k in range(8):
                c = ft["cls"][int(pts[k, 1]), int(pts[k, 0])]
                out[r][i, c] += np.uint8(1)   # uint8 arithmetic: wraps modulo 256

    with np.errstate(over="ignore"):
        for m in listed:
            for x, fx in frames.items():
                if x in listed or fx["marginalized"]:
                    continue
                one_direction(m, x)
                one_direction(x, m)
    return out, pairs, near


def semantic_type(counts, weights=None):
    """semanticTypeId: without a legend the first maximal count; with one the first i with the strictly largest count * weight, the
    first maximal count when every product is 0"""
    counts = np.asarray(counts, dtype=np.uint8)
    first_max = int(np.argmax(counts))
    if weights is None:
        return first_max
    best, best_w = 0, 0
    for i in range(256):
        w = (int(counts[i]) * int(weights[i])) & 0xFFFFFFFFFFFFFFFF   # size_t arithmetic
        if w > best_w:
            best, best_w = i, w
    return first_max if best_w == 0 else best


def semantic_types(hist, weights=None):
    return np.array([semantic_type(row, weights) for row in hist], dtype=np.uint8)


def default_legend_weights():
    """SemanticLegend::weights_ before any tag is read: std::array<size_t, 256> weights_ = {1} — only code 0 has a default weight"""
    w = np.zeros(256, dtype=np.uint64)
    w[0] = 1
    return w
