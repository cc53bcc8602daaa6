"""tests/rotation_ransac_model.py, the NumPy statement of the bootstrap's pure-rotation RANSAC (include/dsopp_hip.h,
dsopp_hip_rotation_ransac_estimate), pinned on the CPU: the solver on noise-free rotations, the det(Q) < 0 flip, the selection walk against
a literal transcription of the reference's loop, the ROI rules and the two decisions.  tests/test_gpu_rotation_ransac.py holds the device
to the model."""
import os
import subprocess

import numpy as np
import pytest

import rotation_ransac_model as rrm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = rrm.Camera(448.0, 448.0, 320.0, 240.0, 640, 480)
ROTATION = rrm.exp_so3([0.01, -0.02, 0.005])


def clean_scene(n, seed=3):
    """A well inside the ROI and B = A rotated, without noise: B stays inside the ROI too"""
    rng = np.random.default_rng(seed)
    A = np.stack([rng.uniform(40, 600, n), rng.uniform(40, 440, n)], axis=1)
    return A, rrm.rotate_points(CAM, ROTATION, A)


def draw_triples(rng, n, count):
    return np.array([rng.choice(n, 3, replace=False) for _ in range(count)], np.int32)


def reference_loop(counts, valid_solution, n, tolerance=0.95):
    """ransac.hpp:36-53 word for word over given findBest results: counts[i] stands for inliers.size() of iteration i"""
    best_inliers, best_solution, i = 0, None, 0
    while i < len(counts) and (np.float64(best_inliers) / np.float64(n) if n else np.float64("nan")) < tolerance:
        inliers, solution = counts[i], valid_solution[i]
        if solution is not None and inliers > best_inliers:
            best_inliers, best_solution = inliers, solution
        i += 1
    return i, best_solution, best_inliers


def test_noise_free_rotation_is_recovered_by_every_hypothesis():
    A, B = clean_scene(200)
    samples = draw_triples(np.random.default_rng(1), len(A), 50)
    res, h = rrm.ransac(CAM, A, B, samples)
    assert h.valid.all()
    assert np.abs(h.rotations - ROTATION).max() <= 1e-12
    assert (h.counts == len(A)).all()
    assert res.iterations_run == 1 and res.best_iteration == 0 and res.inlier_count == len(A)
    assert np.array_equal(res.inliers, np.arange(len(A))) and res.matches == len(A)


def test_negative_determinant_flips_the_whole_matrix():
    """a mirrored sample: Q = V U^T has determinant -1; the solver returns -Q, a rotation, where Kabsch (scipy's align_vectors) corrects
    the last singular direction only"""
    from scipy.spatial.transform import Rotation
    a = np.array([[100.0, 100.0], [500.0, 120.0], [300.0, 400.0]])
    b = a.copy()
    b[:, 0] = CAM.width - 1 - b[:, 0]  # mirrored about the vertical axis
    valid, R, S = rrm.solve(CAM, a, b)
    _, Q, _ = rrm.polar_rotation(rrm.sample_matrix(CAM, a, b))
    assert valid and S[2] / S[0] > 1e-3
    assert np.linalg.det(Q) < -0.5
    assert np.abs(R + Q).max() <= 1e-15
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(R) - 1) <= 1e-14
    ua, ub = rrm.unproject(CAM, a), rrm.unproject(CAM, b)
    ua /= np.linalg.norm(ua, axis=1)[:, None]
    ub /= np.linalg.norm(ub, axis=1)[:, None]
    kabsch = Rotation.align_vectors(ub, ua)[0].as_matrix()  # the rotation that best maps bearings of a onto bearings of b
    assert np.abs(kabsch - R).max() > 0.1
    # the statement of the difference: Kabsch is V diag(1, 1, -1) U^T here
    U, _, Vt = np.linalg.svd(rrm.sample_matrix(CAM, a, b))
    assert np.abs(kabsch - Vt.T @ np.diag([1.0, 1.0, -1.0]) @ U.T).max() <= 1e-9


COUNT_LISTS = [
    ([3, 5, 5, 4, 7, 7], 10),            # ties: the earlier one stays
    ([1, 2, 95, 99, 100], 100),          # 0.95 n reached mid-way: the walk stops before the fourth
    ([1, 2, 94, 99, 100], 100),          # one short of it
    ([0, 0, 0, 0], 10),                  # nothing exceeds 0
    ([5, 4, 3], 5),                      # the first is already everything
    ([], 10),
    ([2, 2], 0),                         # n = 0: 0 / 0 < 0.95 is false, no iteration
]


@pytest.mark.parametrize("counts,n", COUNT_LISTS)
def test_selection_walk_is_the_reference_loop(counts, n):
    run, best_i, best = rrm.select(counts, n)
    ref_run, ref_solution, ref_best = reference_loop(counts, list(range(len(counts))), n)
    assert run == ref_run and best == ref_best
    assert best_i == (-1 if ref_solution is None else ref_solution)


def test_selection_walk_values():
    assert rrm.select([3, 5, 5, 4, 7, 7], 10) == (6, 4, 7)
    assert rrm.select([1, 2, 95, 99, 100], 100) == (3, 2, 95)
    assert rrm.select([1, 2, 94, 99, 100], 100) == (4, 3, 99)
    assert rrm.select([0, 0, 0, 0], 10) == (4, -1, 0)
    assert rrm.select([2, 2], 0) == (0, -1, 0)


def invalid_head_scene():
    """identity data: A == B, so the identity explains every point whose A is inside the ROI; triples 0 and 1 hold a point outside"""
    rng = np.random.default_rng(5)
    A = np.stack([rng.uniform(40, 600, 30), rng.uniform(40, 440, 30)], axis=1)
    A[0] = (2.0, 100.0)  # outside the ROI
    return A, A.copy(), np.array([[0, 1, 2], [3, 0, 4], [5, 6, 7], [8, 9, 10]], np.int32)


def invalid_after_valid_scene():
    """noisy rotated data; triples 1 and 3 hold the point outside the ROI and follow a valid one"""
    rng = np.random.default_rng(6)
    A, B = clean_scene(40)
    B = B + rng.normal(0, 0.6, B.shape)
    A[0] = (2.0, 100.0)
    return A, B, np.array([[1, 2, 3], [0, 4, 5], [6, 7, 8], [0, 9, 10], [11, 12, 13]], np.int32)


def outside_roi_scene():
    """20 clean pairs, then three pairs whose A is outside the ROI (20 .. 22) and one whose B is (23)"""
    A, B = clean_scene(20)
    A = np.vstack([A, [[3.9, 100.0], [300.0, 476.0], [np.nan, 50.0]]])
    B = np.vstack([B, rrm.rotate_points(CAM, ROTATION, np.array([[3.9, 100.0], [300.0, 476.0]])), [[10.0, 10.0]]])
    far = rrm.rotate_points(CAM, ROTATION.T, np.array([[1.0, 1.0]]))  # its rotation lands at (1, 1), outside the ROI, where B is
    return np.vstack([A, far]), np.vstack([B, [[1.0, 1.0]]])


def test_invalid_hypotheses_ahead_of_the_first_valid_one_score_the_identity():
    A, B, samples = invalid_head_scene()
    res, h = rrm.ransac(CAM, A, B, samples)
    assert list(h.valid) == [False, False, True, True]
    assert np.array_equal(h.rotations[0], np.eye(3)) and np.array_equal(h.rotations[1], np.eye(3))
    assert h.counts[0] == h.counts[1] == 29  # every point but the one outside the ROI
    assert res.best_iteration == 0 and res.iterations_run == 1 and np.array_equal(res.rotation, np.eye(3))
    assert 0 not in res.inliers


def test_invalid_hypothesis_after_a_valid_one_never_wins():
    A, B, samples = invalid_after_valid_scene()
    res, h = rrm.ransac(CAM, A, B, samples, tolerance=2.0)
    assert list(h.valid) == [True, False, True, False, True]
    assert np.array_equal(h.rotations[1], h.rotations[0]) and h.counts[1] == h.counts[0]
    assert np.array_equal(h.rotations[3], h.rotations[2]) and h.counts[3] == h.counts[2]
    assert h.valid[res.best_iteration] and res.iterations_run == 5
    # the reference's loop over the same findBest results gives the same winner
    _, ref_solution, ref_best = reference_loop(list(h.counts), list(range(5)), len(A), 2.0)
    assert ref_solution == res.best_iteration and ref_best == res.inlier_count


def test_points_outside_the_roi():
    A, B = outside_roi_scene()
    assert rrm.roi(CAM, A[-1:]).all() and not rrm.roi(CAM, B[-1:]).any()
    d = rrm.distances(CAM, ROTATION, A, B)
    mask = rrm.inlier_mask(d, 1.5)
    assert mask[:20].all()
    assert not mask[20:23].any() and np.isnan(d[20:23]).all()  # never an inlier, although the first two reproject exactly
    assert mask[23] and d[23] < 1e-9                            # B outside the ROI is still compared


def test_roi_edges():
    w, h = CAM.width, CAM.height
    inside = np.array([[4.0, 4.0], [w - 5.0, h - 5.0], [4.0, h - 5.0], [w - 5.0, 4.0]])
    assert rrm.roi(CAM, inside).all()
    outside = np.array([[np.nextafter(4.0, 0.0), 100.0], [np.nextafter(w - 5.0, 1e9), 100.0], [100.0, np.nextafter(4.0, 0.0)],
                        [100.0, np.nextafter(h - 5.0, 1e9)]])
    assert not rrm.roi(CAM, outside).any()


DECISIONS = [
    # previous_frames, inliers, matches -> needNewFrame
    (0, 100, 100, rrm.KEEP_FRAME),   # the first frame is kept whatever the counts
    (1, 71, 100, rrm.DROP_FRAME),
    (1, 70, 100, rrm.KEEP_FRAME),    # inliers == (size_t)(0.7 * 100) = 70: not greater
    (1, 7, 10, rrm.KEEP_FRAME),      # (size_t)(0.7 * 10) = 7
    (1, 8, 10, rrm.DROP_FRAME),
    (1, 2, 3, rrm.KEEP_FRAME),       # (size_t)(2.0999999999999996) = 2
    (1, 3, 3, rrm.DROP_FRAME),
    (1, 0, 0, rrm.KEEP_FRAME),
    (1, 1, 1, rrm.DROP_FRAME),       # (size_t)(0.7) = 0
    (3, 10, 100, rrm.KEEP_FRAME),    # 5 <= 3 + 1 is false
    (4, 10, 100, rrm.FINISH),
    (4, 90, 100, rrm.DROP_FRAME),    # the drop comes first
    (7, 10, 100, rrm.FINISH),
]


@pytest.mark.parametrize("previous,inliers,matches,expected", DECISIONS)
def test_need_new_frame(previous, inliers, matches, expected):
    assert rrm.need_new_frame(previous, inliers, matches) == expected
    assert (inliers == int(0.7 * matches)) <= (rrm.need_new_frame(previous, inliers, matches) != rrm.DROP_FRAME)


def test_standstill_ratio():
    assert rrm.is_standstill(71, 100) and not rrm.is_standstill(70, 100)
    assert not rrm.is_standstill(7, 10) and rrm.is_standstill(8, 10)
    assert not rrm.is_standstill(0, 0)  # 0 / 0 is NaN
    # the two rules differ at the truncation edge: 2 of 3 is no drop (2 > 2 is false) and no standstill (0.667 > 0.7 is false),
    # 1 of 1 is both
    assert rrm.need_new_frame(1, 1, 1) == rrm.DROP_FRAME and rrm.is_standstill(1, 1)


def test_no_cpu_fallback():
    from dsopp_amd import capi
    if capi.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(capi.HipError) as e:
        capi.RotationRansac()
    assert "no HIP device" in str(e.value) or "-4" in str(e.value)


def build_example(tmp_path):
    libdir = os.path.join(ROOT, "dsopp_amd", "lib")
    exe = str(tmp_path / "example_rotation_ransac")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "dsopp_amd", "host", "example_rotation_ransac.cpp"),
                           f"-L{libdir}", "-ldsopp_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", exe])
    return exe


def test_example_driver_compiles_and_fails_loudly_without_gpu(tmp_path):
    from dsopp_amd import capi
    exe = build_example(tmp_path)
    if capi.device_count() > 0:
        pytest.skip("GPU present: tests/test_gpu_rotation_ransac.py runs it")
    r = subprocess.run([exe, "/nonexistent"], capture_output=True, text=True)
    assert r.returncode == 2 and "no CPU fallback" in r.stdout
