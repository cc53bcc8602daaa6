"""The NumPy statement of the marginalisation strategies (include/dsopp_hip.h, dsopp_hip_window_choose_marginalization) and of the
landmarks' count of successful optimisations (dsopp_hip_window_note_optimization), written from the reference:

  SparseFrameMarginalizationStrategy       src/marginalization/src/sparse_frame_marginalization_strategy.cpp:16-168
  MaximumSizeFrameMarginalizationStrategy  src/marginalization/src/maximum_size_frame_marginalization_strategy.cpp:16-20
  ActiveOdometryTrack::marginalizeFrame    src/track/track/src/active_odometry_track.cpp:70-75
  ActiveKeyframe::marginalize              src/track/frames/src/active_keyframe.cpp:176-184
  ActiveTrackingLandmark                   src/track/landmarks/src/active_tracking_landmark.cpp:42-63
  ImmatureTrackingLandmark::readyForActivation  src/track/landmarks/src/immature_tracking_landmark.cpp:46-52

Everything is binary64 and serial, in the reference's order.  tests/test_marginalization_model.py pins it on hand-worked cases,
tests/test_gpu_marginalization.py holds the device to it.

A frame is a dict of the ACTIVE frame's state (track.activeFrames(), oldest first):
  camera_id   the id of the age test
  t           tWorldAgent().translation()
  flags       uint8 per landmark: bit0 isMarginalized, bit1 isOutlier
  n_inliers   numberOfInlierResidualsInTheLastOptimization
  successes   numberOfSuccessfulOptimizations
  idepth, variance
  status_last statuses towards the last active keyframe (0 = kOk), possibly shorter than the frame, or None: a landmark without an entry
              counts as not kOk (the reference would throw)
  immature    None, or dict(status, idepth_min, idepth_max, uniqueness, search_pixel_interval)"""
from collections import namedtuple

import numpy as np

SPARSE, MAXIMUM_SIZE = 0, 1
Options = namedtuple("Options", "strategy minimum_size maximum_size maximum_share_marginalized", defaults=(SPARSE, 5, 7, 0.95))
Result = namedtuple("Result", "selected marginalized scores n_kept n_gone flags n_newly_marginalized n_newly_outlier")

K_EPS = 1e-5
KEEP_FRAMES_FROM_START = 2
MIN_FRAME_AGE = 1
MARGINALIZED, OUTLIER = 1, 2
IMMATURE_READY_STATUSES = (0, 3, 4, 1)  # kGood, kSkipped, kIllConditioned, kOutOfBoundary


def note_optimization(successes, flags, n_inliers):
    """setNumberOfInlierResidualsInTheLastOptimization for every landmark that is not marginalised (photometric_bundle_adjustment.cpp:232,256)"""
    successes = np.asarray(successes).copy()
    successes[((np.asarray(flags) & MARGINALIZED) == 0) & (np.asarray(n_inliers) > 3)] += 1
    return successes


def ready_for_activation(imm):
    idepth = np.asarray(imm["idepth_max"], np.float64) * 0.5 + np.asarray(imm["idepth_min"], np.float64) * 0.5
    return (np.isin(imm["status"], IMMATURE_READY_STATUSES) & (np.asarray(imm["search_pixel_interval"]) < 8.0) &
            (np.asarray(imm["uniqueness"]) > 3.0) & (idepth > 0))


def counts(frame):
    """(numberOfActiveAndImmatureLandmarks, numberOfMarginalizedLandmarks), :16-35"""
    gone = (np.asarray(frame["flags"]) & (MARGINALIZED | OUTLIER)) != 0
    kept = int(np.count_nonzero(~gone))
    if frame.get("immature") is not None:
        kept += int(np.count_nonzero(ready_for_activation(frame["immature"])))
    return kept, int(np.count_nonzero(gone))


def distance(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])


def scores_of(frames):
    """distance_score of every candidate of findFramesToMarginalize (:110-130); NaN where the loop skips the frame or never reaches it"""
    A = len(frames)
    out = np.full(A, np.nan)
    last = frames[-1]
    for r in range(max(0, A - KEEP_FRAMES_FROM_START)):
        ref = frames[r]
        if ref["camera_id"] + MIN_FRAME_AGE > last["camera_id"]:
            continue
        score = np.float64(0)
        for t in range(A - KEEP_FRAMES_FROM_START):
            if frames[t]["camera_id"] + MIN_FRAME_AGE > last["camera_id"] + 1 or r == t:
                continue
            score = score + 1 / (K_EPS + distance(ref["t"], frames[t]["t"]))
        out[r] = score * np.sqrt(distance(ref["t"], last["t"]))
    return out


def erase_order(selected, A):
    """marginalizeFrame(idx) for idx ascending over the set, against the list as it shrinks (:165-167): the active indices hit"""
    alive = list(range(A))
    hit = []
    for idx in sorted(selected):
        if idx < len(alive):  # (past the end: undefined in the reference)
            hit.append(alive.pop(idx))
    return hit


def marginalize_landmark(flag, variance, idepth):
    """ActiveTrackingLandmark::marginalize (:55-63) on a flag byte"""
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.float64(variance) / np.float64(idepth)
    if q > 1e-3 or idepth < 0:
        flag |= OUTLIER
    return flag | MARGINALIZED


def choose(frames, options=Options()):
    A = len(frames)
    kept_gone = [counts(f) for f in frames]
    scores = np.full(A, np.nan)
    flags = [np.asarray(f["flags"], np.uint8).copy() for f in frames]
    selected = set()
    if A == 0:
        return Result([], [], scores, [], [], flags, 0, 0)
    if options.strategy == SPARSE:
        # findFramesWithSmallNumberOfActivePoints (:38-53): the size test reads the set as it grows
        for i in range(max(0, A - KEEP_FRAMES_FROM_START)):
            kept, gone = np.float64(kept_gone[i][0]), np.float64(kept_gone[i][1])
            if kept < (1 - options.maximum_share_marginalized) * (kept + gone) and A - len(selected) > options.minimum_size:
                selected.add(i)
        # findFramesToMarginalize (:101-140)
        if A > options.maximum_size + len(selected):
            scores = scores_of(frames)
            max_score, chosen = 0.0, 0
            for r in range(A):
                if scores[r] > max_score:  # (NaN compares false)
                    max_score, chosen = scores[r], r
            selected.add(chosen)
        # marginalizeLandmarks (:56-91)
        if A > KEEP_FRAMES_FROM_START:
            min_good = (options.minimum_size + 1) // 2
            good_optimizations = 2 * options.maximum_size
            for a in range(A - 1):
                f = frames[a]
                status = f.get("status_last")
                for i in range(len(flags[a])):
                    if flags[a][i] & (MARGINALIZED | OUTLIER):
                        continue
                    ok = status is not None and i < len(status) and status[i] == 0
                    out_of_boundary = (a in selected) or not ok
                    valid = f["n_inliers"][i] >= min_good and f["successes"][i] > good_optimizations
                    sufficient = f["successes"][i] > 0
                    if out_of_boundary and not sufficient:
                        flags[a][i] |= OUTLIER
                    elif out_of_boundary or valid:
                        flags[a][i] = marginalize_landmark(flags[a][i], f["variance"][i], f["idepth"][i])
        order = sorted(selected)
        hit = erase_order(order, A)
    else:
        hit = list(range(max(0, A - options.maximum_size)))  # marginalizeFrame(0) until the size fits
        order = list(hit)
    for a in hit:  # ActiveKeyframe::marginalize: every landmark, whatever its flags
        for i in range(len(flags[a])):
            flags[a][i] = marginalize_landmark(flags[a][i], frames[a]["variance"][i], frames[a]["idepth"][i])
    newly_marg = sum(int(np.count_nonzero((n & MARGINALIZED) & ~(np.asarray(f["flags"], np.uint8) & MARGINALIZED))) for n, f in zip(flags, frames))
    newly_outl = sum(int(np.count_nonzero((n & OUTLIER) & ~(np.asarray(f["flags"], np.uint8) & OUTLIER))) for n, f in zip(flags, frames))
    return Result(order, hit, scores, [k for k, _ in kept_gone], [g for _, g in kept_gone], flags, newly_marg, newly_outl)
