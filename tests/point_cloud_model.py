"""NumPy statement of the map (include/dsopp_hip.h, "the map"; dsopp_amd/csrc/point_cloud.hip): the update of a keyframe's landmark records
from a window's values and the export of the records as a point cloud.  Serial, binary64, every arithmetic step a single IEEE operation
in the order the header states, record after record in the reference's order:
  PhotometricBundleAdjustment::updateFrame      src/energy/problems/src/photometric_bundle_adjustment.cpp:223-263
  ActiveTrackingLandmark::marginalize           src/track/landmarks/src/active_tracking_landmark.cpp:55-63
  validForVisualization / getColor              src/track/frames/src/frame.cpp:19-82
  initializeVisiblePointsStorage                src/output/visualizer/src/local_track.cpp:139-158
  the exporter's loop                           pydsopp/utils/point_cloud_exporter.py:83-107
tests/test_point_cloud_model.py pins it on hand-worked cases; tests/test_gpu_point_cloud.py holds the kernels to it exactly."""
import dataclasses

import numpy as np

FLAG_MARGINALIZED, FLAG_OUTLIER = 1, 2            # a record's flags (DSOPP_HIP_MAP_FLAG_*)
WINDOW_MARGINALIZED, WINDOW_OUTLIER = 1, 2        # the window's landmark flag bits
CLASS_ACTIVE, CLASS_MARGINALIZED, CLASS_OUTLIER = 1, 2, 4
CLASS_ALL = 7
FRAME_KEYFRAME, FRAME_WORLD = 0, 1
COLOURS_LANDMARK_TYPE, COLOURS_CONSTANT, COLOURS_SEMANTIC, COLOURS_IMAGE = 0, 1, 2, 3

DBL_MAX = np.finfo(np.float64).max
IDEPTH_EPS = 1e-8                      # kIdepthEps of updateFrame
MAX_RELATIVE_IDEPTH_VARIANCE = 1e-3    # marginalize()
MIN_HOMOGENEOUS = 1e-16                # the exporter's skip
EXPORTER_MAX_IDEPTH_VARIANCE, EXPORTER_MIN_RELATIVE_BASELINE = 5e-8, 0.15

# kSemanticColors, frame.cpp:19-26
SEMANTIC_COLOURS = np.array([(200, 200, 200), (71, 71, 107), (255, 77, 210), (255, 255, 153), (255, 0, 0), (51, 51, 153), (224, 224, 235),
                             (255, 255, 0), (127, 127, 127), (0, 255, 0), (0, 0, 255), (102, 51, 0), (51, 102, 153), (139, 0, 255)], dtype=np.uint8)
COLOUR_OUTLIER, COLOUR_MARGINALIZED, COLOUR_ACTIVE = (255, 0, 0), (255, 100, 100), (100, 255, 100)
COLOUR_CONSTANT = (200, 200, 200)


class StateError(RuntimeError):
    """what the library reports as DSOPP_HIP_ERR_STATE"""


@dataclasses.dataclass
class Keyframe:
    frame_id: int
    intrinsics: np.ndarray                  # fx, fy, cx, cy
    pose: np.ndarray                        # qx, qy, qz, qw, tx, ty, tz
    has_image: bool = False
    live: bool = True
    uv: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros((0, 2)))
    idepth: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros(0))
    variance: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros(0))
    relative_baseline: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros(0))
    flags: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros(0, dtype=np.uint8))
    type: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros(0, dtype=np.uint8))
    rgb: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros((0, 3), dtype=np.uint8))

    @property
    def n(self):
        return len(self.idepth)

    def copy(self):
        return dataclasses.replace(self, **{f.name: np.array(getattr(self, f.name)) for f in dataclasses.fields(self)
                                            if isinstance(getattr(self, f.name), np.ndarray)})


def keyframe_from_records(frame_id, intrinsics, pose, uv, idepth, variance, relative_baseline, flags, type=None, rgb=None):
    """dsopp_hip_map_set_records: a finalised keyframe from arrays"""
    n = len(idepth)
    return Keyframe(frame_id, np.asarray(intrinsics, dtype=np.float64), np.asarray(pose, dtype=np.float64), has_image=rgb is not None, live=False,
                    uv=np.asarray(uv, dtype=np.float64).reshape(n, 2), idepth=np.asarray(idepth, dtype=np.float64),
                    variance=np.asarray(variance, dtype=np.float64), relative_baseline=np.asarray(relative_baseline, dtype=np.float64),
                    flags=np.asarray(flags, dtype=np.uint8), type=np.zeros(n, dtype=np.uint8) if type is None else np.asarray(type, dtype=np.uint8),
                    rgb=np.zeros((n, 3), dtype=np.uint8) if rgb is None else np.asarray(rgb, dtype=np.uint8).reshape(n, 3))


def semantic_type(hist_row, weights=None):
    """ActiveTrackingLandmark::semanticTypeId (active_tracking_landmark.cpp:71-88); weights = 256 unsigned 64-bit integers or None"""
    best = int(np.argmax(hist_row))  # std::max_element: the first maximal count
    if weights is None:
        return best
    best_w, best_wi = 0, 0
    for i in range(256):
        w = (int(hist_row[i]) * int(weights[i])) & 0xFFFFFFFFFFFFFFFF  # size_t arithmetic
        if w > best_w:
            best_w, best_wi = w, i
    return best if best_w == 0 else best_wi


def sample_colour(image, u, v):
    """the kept image at [int(v), int(u)]: BGR -> RGB, a grey image replicated; (0, 0, 0) without an image or outside it"""
    if image is None:
        return (0, 0, 0)
    h, w = image.shape[:2]
    if not (0.0 <= u < w and 0.0 <= v < h):
        return (0, 0, 0)
    px = image[int(v), int(u)]
    if image.ndim == 3:
        return (int(px[2]), int(px[1]), int(px[0]))
    return (int(px),) * 3


def update_keyframe(kf, uv, idepth, inv_hessian_idepth, relative_baseline, flags, hist=None, image=None, weights=None, estimate_uncertainty=True,
                    channels=1):
    """dsopp_hip_map_update for one keyframe, in place: the window's values of its landmarks in the caller's order (hist: n x 256 class
    counters or None = no observation has reached the frame)"""
    n = len(idepth)
    assert n >= kf.n
    uv = np.asarray(uv, dtype=np.float64).reshape(n, 2)
    grow = n - kf.n
    first_new = kf.n
    kf.uv = np.concatenate([kf.uv, np.zeros((grow, 2))])
    kf.idepth = np.concatenate([kf.idepth, np.zeros(grow)])
    kf.variance = np.concatenate([kf.variance, np.zeros(grow)])
    kf.relative_baseline = np.concatenate([kf.relative_baseline, np.zeros(grow)])
    kf.flags = np.concatenate([kf.flags, np.zeros(grow, dtype=np.uint8)])
    kf.type = np.concatenate([kf.type, np.zeros(grow, dtype=np.uint8)])
    kf.rgb = np.concatenate([kf.rgb, np.zeros((grow, 3), dtype=np.uint8)])
    C = np.float64(channels)
    with np.errstate(all="ignore"):
        for i in range(n):
            w_idepth, w_flags = np.float64(idepth[i]), int(flags[i])
            if i >= first_new:  # 1 a new record
                kf.uv[i] = uv[i]
                kf.idepth[i] = w_idepth
                kf.variance[i] = DBL_MAX
                kf.relative_baseline[i] = 0.0
                kf.flags[i] = 0
                kf.type[i] = 0
                kf.rgb[i] = sample_colour(image, uv[i, 0], uv[i, 1])
            if w_flags & WINDOW_OUTLIER:  # 2 (:229-231)
                kf.flags[i] |= FLAG_OUTLIER
            if not w_flags & WINDOW_MARGINALIZED:  # 3 (:232-260)
                if abs(w_idepth) < IDEPTH_EPS:
                    kf.idepth[i] = 0.0
                elif w_idepth < 0:
                    kf.flags[i] |= FLAG_OUTLIER
                else:
                    kf.idepth[i] = w_idepth
                kf.variance[i] = np.float64(inv_hessian_idepth[i]) * C if estimate_uncertainty else 1e-5
                if relative_baseline[i] > kf.relative_baseline[i]:
                    kf.relative_baseline[i] = relative_baseline[i]
            elif not kf.flags[i] & FLAG_MARGINALIZED:  # 4 marginalize()
                if kf.variance[i] / kf.idepth[i] > MAX_RELATIVE_IDEPTH_VARIANCE or kf.idepth[i] < 0:
                    kf.flags[i] |= FLAG_OUTLIER
                kf.flags[i] |= FLAG_MARGINALIZED
            if hist is not None:  # 5
                kf.type[i] = semantic_type(hist[i], weights)
    return kf


def rotation(q):
    """(qx, qy, qz, qw) -> R by the formula of dsopp_amd.synthetic.params_to_mat"""
    x, y, z, w = (np.float64(c) for c in q[:4])
    return np.array([
        [1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
        [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
        [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)],
    ], dtype=np.float64)


def record_class(flags):
    if flags & FLAG_OUTLIER:
        return CLASS_OUTLIER
    return CLASS_MARGINALIZED if flags & FLAG_MARGINALIZED else CLASS_ACTIVE


def passes(idepth, variance, relative_baseline, flags, classes=CLASS_ALL, apply_filters=False, max_idepth_variance=EXPORTER_MAX_IDEPTH_VARIANCE,
           min_relative_baseline_filter=EXPORTER_MIN_RELATIVE_BASELINE, frame=FRAME_WORLD, min_relative_baseline=0.1):
    """validForVisualization by class mask, the two strict filters, the exporter's skip"""
    ok = idepth != 0 and relative_baseline > min_relative_baseline and bool(classes & record_class(int(flags)))
    if apply_filters:
        ok = ok and variance < max_idepth_variance and relative_baseline > min_relative_baseline_filter
    if frame == FRAME_WORLD:
        ok = ok and not abs(idepth) < MIN_HOMOGENEOUS
    return bool(ok)


def direction(intrinsics, u, v):
    """d = ((u - cx) (1 / fx), (v - cy) (1 / fy), 1)"""
    fx, fy, cx, cy = (np.float64(c) for c in intrinsics)
    ifx, ify = np.float64(1.0) / fx, np.float64(1.0) / fy
    return (np.float64(u) - cx) * ifx, (np.float64(v) - cy) * ify


def position(intrinsics, R, t, u, v, idepth, frame):
    dx, dy = direction(intrinsics, u, v)
    idepth = np.float64(idepth)
    if frame == FRAME_KEYFRAME:
        return dx / idepth, dy / idepth, np.float64(1.0) / idepth
    return tuple((((R[i, 0] * dx + R[i, 1] * dy) + R[i, 2]) + np.float64(t[i]) * idepth) / idepth for i in range(3))


def colour(scheme, flags, type, rgb):
    if scheme == COLOURS_LANDMARK_TYPE:
        return {CLASS_OUTLIER: COLOUR_OUTLIER, CLASS_MARGINALIZED: COLOUR_MARGINALIZED, CLASS_ACTIVE: COLOUR_ACTIVE}[record_class(int(flags))]
    if scheme == COLOURS_CONSTANT:
        return COLOUR_CONSTANT
    if scheme == COLOURS_SEMANTIC:
        return tuple(SEMANTIC_COLOURS[int(type) % 14])
    assert scheme == COLOURS_IMAGE, scheme
    return tuple(rgb)


def export(keyframes, classes=CLASS_ACTIVE | CLASS_MARGINALIZED, apply_filters=False, max_idepth_variance=EXPORTER_MAX_IDEPTH_VARIANCE,
           min_relative_baseline_filter=EXPORTER_MIN_RELATIVE_BASELINE, frame=FRAME_WORLD, colours=COLOURS_LANDMARK_TYPE, min_relative_baseline=0.1):
    """dsopp_hip_map_export over `keyframes` in their order: dict of packed arrays, count and per_keyframe_counts"""
    if colours == COLOURS_IMAGE:
        for kf in keyframes:
            if not kf.has_image:
                raise StateError(f"keyframe {kf.frame_id} has no image colours")
    xyz, rgb, types, baselines, variances, kf_index, rec_index, per_kf = [], [], [], [], [], [], [], []
    with np.errstate(all="ignore"):
        for k, kf in enumerate(keyframes):
            R, t = rotation(kf.pose), kf.pose[4:7]
            before = len(xyz)
            for i in range(kf.n):
                if not passes(kf.idepth[i], kf.variance[i], kf.relative_baseline[i], kf.flags[i], classes, apply_filters, max_idepth_variance,
                              min_relative_baseline_filter, frame, min_relative_baseline):
                    continue
                xyz.append(position(kf.intrinsics, R, t, kf.uv[i, 0], kf.uv[i, 1], kf.idepth[i], frame))
                rgb.append(colour(colours, kf.flags[i], kf.type[i], kf.rgb[i]))
                types.append(kf.type[i])
                baselines.append(kf.relative_baseline[i])
                variances.append(kf.variance[i])
                kf_index.append(k)
                rec_index.append(i)
            per_kf.append(len(xyz) - before)
    n = len(xyz)
    return dict(xyz=np.array(xyz, dtype=np.float64).reshape(n, 3), rgb=np.array(rgb, dtype=np.uint8).reshape(n, 3), type=np.array(types, dtype=np.uint8),
                relative_baseline=np.array(baselines, dtype=np.float64), idepth_variance=np.array(variances, dtype=np.float64),
                keyframe_index=np.array(kf_index, dtype=np.int32), record_index=np.array(rec_index, dtype=np.int32), count=n,
                per_keyframe_counts=np.array(per_kf, dtype=np.int32))
