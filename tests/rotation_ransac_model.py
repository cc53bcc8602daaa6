"""The NumPy statement of the bootstrap's pure-rotation RANSAC (include/dsopp_hip.h, dsopp_hip_rotation_ransac_estimate): the three-point
rotation solver with numpy.linalg.svd, the inlier test, the rule for invalid hypotheses, the selection walk, and the two decisions that
consume the inlier count.  Everything is binary64.  tests/test_rotation_ransac.py pins it on the CPU, tests/test_gpu_rotation_ransac.py
holds the device to it.

A is the NEW frame's points, B the last bootstrap keyframe's; a hypothesis' rotation maps bearings of A onto bearings of B."""
from collections import namedtuple

import numpy as np

Camera = namedtuple("Camera", "fx fy cx cy width height")
Hypotheses = namedtuple("Hypotheses", "valid rotations counts distances sigma")
Result = namedtuple("Result", "iterations_run best_iteration rotation inlier_count inliers matches")

DROP_FRAME, KEEP_FRAME, FINISH = "drop", "keep", "finish"


def roi(cam, p):
    """camera_model_base.hpp:53-60, per row of p; a NaN is outside"""
    p = np.asarray(p, np.float64).reshape(-1, 2)
    return (p[:, 0] >= 4.0) & (p[:, 0] <= cam.width - 5.0) & (p[:, 1] >= 4.0) & (p[:, 1] <= cam.height - 5.0)


def unproject(cam, p):
    p = np.asarray(p, np.float64).reshape(-1, 2)
    return np.stack([(p[:, 0] - cam.cx) / cam.fx, (p[:, 1] - cam.cy) / cam.fy, np.ones(len(p))], axis=1)


def sample_matrix(cam, a, b):
    """H = sum_k a_k b_k^T / 9 over the normalised bearings of a sample (3 x 2 each)"""
    ua, ub = unproject(cam, a), unproject(cam, b)
    ua /= np.linalg.norm(ua, axis=1)[:, None]
    ub /= np.linalg.norm(ub, axis=1)[:, None]
    return sum(np.outer(ua[k], ub[k]) for k in range(3)) / 9.0


def polar_rotation(H):
    """(R, Q, singular values): H = U S V^T, Q = V U^T, R = det(Q) Q — the whole matrix flips, not Kabsch's diag(1, 1, d)"""
    U, S, Vt = np.linalg.svd(H)
    Q = Vt.T @ U.T
    return np.linalg.det(Q) * Q, Q, S


def solve(cam, a, b):
    """PureRorationSolver::solve of one sample: (valid, R, singular values); an invalid sample has no rotation of its own"""
    if not (roi(cam, a).all() and roi(cam, b).all()):
        return False, None, None
    R, _, S = polar_rotation(sample_matrix(cam, a, b))
    return True, R, S


def distances(cam, R, A, B):
    """per pair |project(R unproject(A[j])) - B[j]|, NaN where A[j] is outside the ROI (such a point is never an inlier)"""
    A, B = np.asarray(A, np.float64).reshape(-1, 2), np.asarray(B, np.float64).reshape(-1, 2)
    u = unproject(cam, A)
    with np.errstate(all="ignore"):
        x = R[0, 0] * u[:, 0] + R[0, 1] * u[:, 1] + R[0, 2]
        y = R[1, 0] * u[:, 0] + R[1, 1] * u[:, 1] + R[1, 2]
        z = R[2, 0] * u[:, 0] + R[2, 1] * u[:, 1] + R[2, 2]
        dx = cam.fx * x / z + cam.cx - B[:, 0]
        dy = cam.fy * y / z + cam.cy - B[:, 1]
        d = np.sqrt(dx * dx + dy * dy)
    return np.where(roi(cam, A), d, np.nan)


def inlier_mask(d, threshold):
    with np.errstate(invalid="ignore"):
        return d < threshold  # (strict; False for a NaN)


def hypotheses(cam, A, B, samples, threshold):
    """every hypothesis scored: an invalid one carries the rotation and count of its nearest valid predecessor, the identity's ahead of
    the first valid one (the reference scores the solver's previous solution)"""
    A, B = np.asarray(A, np.float64).reshape(-1, 2), np.asarray(B, np.float64).reshape(-1, 2)
    samples = np.asarray(samples, np.int64).reshape(-1, 3)
    m = len(samples)
    valid, rotations = np.zeros(m, bool), np.zeros((m, 3, 3))
    counts, dist, sigma = np.zeros(m, np.int64), np.zeros((m, len(A))), np.full((m, 3), np.nan)
    R = np.eye(3)
    for i, s in enumerate(samples):
        ok, Ri, S = solve(cam, A[s], B[s])
        if ok:
            R, sigma[i] = Ri, S
        valid[i], rotations[i] = ok, R
        dist[i] = distances(cam, R, A, B)
        counts[i] = inlier_mask(dist[i], threshold).sum()
    return Hypotheses(valid, rotations, counts, dist, sigma)


def select(counts, n, tolerance=0.95):
    """the serial loop's meaning over the counts: (iterations_run, best_iteration, best count)"""
    best, best_i, run = 0, -1, 0
    for i, c in enumerate(counts):
        with np.errstate(all="ignore"):
            if not np.float64(best) / np.float64(n) < tolerance:
                break
        run = i + 1
        if c > best:
            best, best_i = int(c), i
    return run, best_i, best


def ransac(cam, A, B, samples, threshold=1.5, tolerance=0.95):
    A = np.asarray(A, np.float64).reshape(-1, 2)
    n = len(A)
    if n == 0:
        return Result(0, -1, np.eye(3), 0, np.zeros(0, np.int64), 0), None
    h = hypotheses(cam, A, B, samples, threshold)
    run, best_i, best = select(h.counts, n, tolerance)
    if best_i < 0:
        return Result(run, -1, np.eye(3), 0, np.zeros(0, np.int64), n), h
    inliers = np.flatnonzero(inlier_mask(h.distances[best_i], threshold))
    return Result(run, best_i, h.rotations[best_i], best, inliers, n), h


def need_new_frame(previous_frames, inliers, matches, sliding_window_length=5, rotation_inlier_ratio=0.7):
    """WaitForMovementInitializerKeyframeStrategy::needNewFrame (wait_for_movement_keyframe_strategy.cpp:13-29), with the
    static_cast<size_t> truncation of the product"""
    if previous_frames == 0:
        return KEEP_FRAME
    if inliers > int(np.float64(rotation_inlier_ratio) * np.float64(matches)):
        return DROP_FRAME
    if sliding_window_length <= previous_frames + 1:
        return FINISH
    return KEEP_FRAME


def is_standstill(inliers, matches, max_ratio=0.7):
    """addNewFrame's test (add_new_frame.cpp:36-45): Precision(inliers) / Precision(matches) > 0.7; 0 / 0 is NaN and no standstill"""
    with np.errstate(all="ignore"):
        return bool(np.float64(inliers) / np.float64(matches) > max_ratio)


def exp_so3(w):
    """Rodrigues' formula"""
    w = np.asarray(w, np.float64)
    t = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if t < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(t) / t * K + (1 - np.cos(t)) / (t * t) * K @ K


def rotate_points(cam, R, A):
    """project(R unproject(A)) per row, with no ROI test"""
    u = unproject(cam, A) @ R.T
    return np.stack([cam.fx * u[:, 0] / u[:, 2] + cam.cx, cam.fy * u[:, 1] / u[:, 2] + cam.cy], axis=1)
