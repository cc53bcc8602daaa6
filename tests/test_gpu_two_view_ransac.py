"""The device's two-view pose (dsopp_amd/csrc/two_view_ransac.hip, capi.TwoViewRansac) against its NumPy statement
(tests/two_view_ransac_model.py).  The bars, from include/dsopp_hip.h and DESIGN.md row i-6, none of them a device result
(tests/test_two_view_ransac.py computes, derives and guards them):
  * per hypothesis: an invalid sample has no solution; on a pinned sample the number of solutions is the model's and every pose lies within
    the sample's bar, max(1e-11, 64 x the model's own change under a 1 +- 2^-52 perturbation of the sample's inputs); at most 5 % of a
    case's samples are unpinned;
  * counts within [sure, sure + near], leaving out every (solution, pair) decision whose model d lies within 1e-3 t_ang of t_ang; at most
    0.1 % of the decisions are left out, and none of a hypothesis that could reach the winner's count, so the winner is determined;
  * best_iteration, best_solution and ransac_inlier_count exactly; pose_ransac within its sample's bar, pose_reselect and pose within
    max(1e-11, 16 x the model's change under the same perturbation of all pairs and of the start);
  * the inlier list exactly, up to pairs in the band; cost_final <= cost_initial in both stages;
  * refine_iterations and refine_flags equal to the model's wherever neither of the model's runs takes a decision on its edge and the winner
    has more than five inliers (five fit exactly: that refinement runs on rounding noise)."""
import ctypes as C
import struct
import subprocess

import numpy as np
import pytest

import geometric_ba_model as gm
import pnp_ransac_model as pm
import test_two_view_ransac as ttv
import two_view_ransac_model as tm

pytestmark = pytest.mark.gpu

CAM = ttv.CAM
T_ANG = ttv.T_ANG


@pytest.fixture(scope="module")
def tv():
    from dsopp_amd import capi
    r = capi.TwoViewRansac()
    yield r
    r.close()


def assert_sane_poses(poses, label, tolerance=1e-8):
    for pose in poses:
        R, t = tm.pose_parts(pose)
        assert np.isfinite(pose).all() and np.abs(R @ R.T - np.eye(3)).max() <= tolerance and abs(np.linalg.det(R) - 1.0) <= tolerance and \
            abs(t @ t - 1.0) <= tolerance, (label, pose)


def assert_hypotheses(got, c, label):
    """validity, number of solutions, poses and counts per hypothesis"""
    h, pinned, bar = c["h"], c["pinned"], c["bar"]
    m = len(c["samples"])
    num = got["hyp_num_solutions"].astype(np.int64)
    assert ((num >= 0) & (num <= tm.MAX_SOLUTIONS)).all(), label
    ok = tm.match_mask(CAM, c["A"], c["B"])
    valid = np.array([bool(ok[s].all()) for s in np.asarray(c["samples"], np.int64).reshape(-1, 5)], bool)
    assert not num[~valid].any(), (label, "an invalid sample has solutions")
    assert np.array_equal(num[pinned], h.num_solutions[pinned]), (label, np.flatnonzero(pinned & (num != h.num_solutions)))
    unused = np.arange(tm.MAX_SOLUTIONS)[None, :] >= num[:, None]
    assert not got["hyp_poses"][unused].any() and not got["hyp_counts"][unused].any(), (label, "an unused slot is not zero")
    assert_sane_poses(got["hyp_poses"][~unused], label)
    if not pinned.any():
        return
    err = np.abs(got["hyp_poses"] - h.poses).max(axis=(1, 2))
    ratio = (err / bar)[pinned]
    print(f"{label}: {int((~pinned).sum())} of {m} samples unpinned; greatest pose difference {err[pinned].max():.3e}, greatest share of a bar {ratio.max():.3f}")
    assert (ratio <= 1.0).all(), (label, int(np.argmax(np.where(pinned, err / bar, 0))), err.max())
    sure, near = c["sure"].sum(axis=2), c["near"].sum(axis=2)
    dev = got["hyp_counts"].astype(np.int64)
    assert ((dev >= sure) & (dev <= sure + near))[pinned].all(), (label, np.flatnonzero(pinned & ((dev < sure) | (dev > sure + near)).any(axis=1)))


def assert_no_winner(got, label):
    for k in ("pose", "pose_reselect", "pose_ransac"):
        assert np.array_equal(got[k], tm.IDENTITY), (label, k)
    assert (got["best_iteration"], got["best_solution"], got["ransac_inlier_count"], got["inlier_count"]) == (-1, -1, 0, 0) and len(got["inliers"]) == 0, label
    assert (got["refine_iterations"], got["refine_flags"], got["cost_initial"], got["cost_final"]) == ((0, 0), (0, 0), (0.0, 0.0), (0.0, 0.0)), label


def assert_result(got, c, label):
    res = c["res"]
    assert got["matches"] == res.matches, label
    assert (got["best_iteration"], got["best_solution"], got["ransac_inlier_count"]) == (res.best_iteration, res.best_solution, res.ransac_inlier_count), label
    if res.best_iteration < 0:
        assert_no_winner(got, label)
        return
    assert np.abs(got["pose_ransac"] - res.pose_ransac).max() <= c["bar"][res.best_iteration], label
    assert got["inliers"].dtype == np.int32 and got["inlier_count"] == len(got["inliers"]) and np.all(np.diff(got["inliers"]) > 0), label
    assert_sane_poses([got["pose_ransac"], got["pose_reselect"], got["pose"]], label, 1e-9)
    for stage in range(2):
        assert 0 <= got["refine_iterations"][stage] <= tm.MAX_ITERATIONS and got["cost_final"][stage] <= got["cost_initial"][stage], (label, stage)
    diffs = np.abs(got["pose_reselect"] - res.pose_reselect).max(), np.abs(got["pose"] - res.pose).max()
    print(f"{label}: pose_reselect off the model by {diffs[0]:.3e} (bar {c['bar_reselect']:.3e}), pose by {diffs[1]:.3e} (bar {c['bar_final']:.3e})")
    assert diffs[0] <= c["bar_reselect"] and diffs[1] <= c["bar_final"], label
    sure, near = ttv.near_decisions(res.distances)
    inl = set(got["inliers"].tolist())
    assert set(np.flatnonzero(sure).tolist()) <= inl <= set(np.flatnonzero(sure | near).tolist()), label
    assert near.sum() <= max(1e-3 * len(c["A"]), 1), label
    if ttv.records_are_compared(res) and not near.any():
        expected = tuple(s.iterations for s in res.stages), tuple(s.flags for s in res.stages)
        assert (got["refine_iterations"], got["refine_flags"]) == expected, (label, got["refine_iterations"], got["refine_flags"], expected)
        for stage in range(2):
            assert abs(got["cost_final"][stage] - res.stages[stage].cost_final) <= 1e-9 * res.stages[stage].cost_final, (label, stage)


def run_case(tv, c, label):
    fig = ttv.check_case_guards(c, label)
    print(f"{label}: {fig}")
    got = tv.estimate(ttv.camera_args(), c["A"], c["B"], c["samples"], min_matches=c["min_matches"], with_hypotheses=True)
    if len(c["samples"]) and c["res"].matches >= c["min_matches"]:
        assert_hypotheses(got, c, label)
    assert_result(got, c, label)
    return got


@pytest.mark.parametrize("n", [5, 6, 63, 64, 65, 257, 500])
def test_pair_counts(tv, n):
    """n = 5: one sample in its orders, an exact fit — the refinement runs on rounding noise and its record is not compared"""
    run_case(tv, ttv.noisy_case(n, 200), f"n = {n}")


@pytest.mark.parametrize("iterations", [0, 1, 3, 4, 5, 200, 256, 1000])
def test_hypothesis_counts(tv, iterations):
    """the wave, workgroup and ticket edges of four waves"""
    got = run_case(tv, ttv.noisy_case(257, iterations), f"{iterations} hypotheses")
    if iterations == 0:
        assert got["best_iteration"] == -1 and got["matches"] == 257


def test_records_are_compared_somewhere():
    compared = [(n, it) for n, it in ttv.GUARDED_CASES if ttv.records_are_compared(ttv.noisy_case(n, it)["res"])]
    assert len(compared) >= 4, compared


def test_two_runs_give_the_same_bytes(tv):
    c = ttv.noisy_case(500, 200)
    a = tv.estimate(ttv.camera_args(), c["A"], c["B"], c["samples"], with_hypotheses=True)
    other = ttv.noisy_case(65, 200)
    tv.estimate(ttv.camera_args(), other["A"], other["B"], other["samples"])            # the buffers are used in between
    b = tv.estimate(ttv.camera_args(), c["A"], c["B"], c["samples"], with_hypotheses=True)
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    plain = tv.estimate(ttv.camera_args(), c["A"], c["B"], c["samples"])
    for k in plain:
        assert np.asarray(a[k]).tobytes() == np.asarray(plain[k]).tobytes(), k


def small_case(A, B, samples, min_matches=5, seed=9):
    A, B, samples = np.asarray(A, np.float64), np.asarray(B, np.float64), np.asarray(samples, np.int32).reshape(-1, 5)
    res, h = tm.estimate(CAM, A, B, samples, min_matches=min_matches)
    pinned, bar, change, route = ttv.pin_samples(A, B, samples, seed)
    sure, near = ttv.near_decisions(h.distances) if len(h.num_solutions) else (np.zeros((len(samples), 10, len(A)), bool),) * 2
    bars = ttv.refinement_bars(CAM, res, A, B, seed + 1) if res.best_iteration >= 0 else (ttv.REFINE_FLOOR, ttv.REFINE_FLOOR, 0.0)
    return dict(A=A, B=B, samples=samples, res=res, h=h, pinned=pinned, bar=bar, change=change, route=route, sure=sure, near=near,
                reselect_near=ttv.near_decisions(res.distances)[1], bar_reselect=bars[0], bar_final=bars[1], min_matches=min_matches)


def test_too_few_matches_leave_the_samples_unread(tv):
    c = ttv.noisy_case(65, 200)
    A = c["A"].copy()
    A[:20, 0] = 2.0                                                       # 45 matches of 65 pairs
    garbage = np.full((7, 5), 12345, np.int32)                            # indices no call may read
    got = tv.estimate(ttv.camera_args(), A, c["B"], garbage, with_hypotheses=True)
    assert got["matches"] == 45
    assert_no_winner(got, "too few matches")
    assert not got["hyp_num_solutions"].any() and not got["hyp_poses"].any() and not got["hyp_counts"].any()
    res, _ = tm.estimate(CAM, A, c["B"], garbage)
    assert res.matches == 45 and res.best_iteration == -1
    got = tv.estimate(ttv.camera_args(), A, c["B"], c["samples"][:40], min_matches=45)    # exactly enough: min_matches is not a strict bound
    assert got["best_iteration"] >= 0


def test_no_pairs(tv):
    got = tv.estimate(ttv.camera_args(), np.zeros((0, 2)), np.zeros((0, 2)), np.zeros((0, 5), np.int32), min_matches=0, with_hypotheses=True)
    assert got["matches"] == 0
    assert_no_winner(got, "n = 0")
    got = tv.estimate(ttv.camera_args(), np.zeros((0, 2)), np.zeros((0, 2)), np.array([[0, 1, 2, 3, 4]], np.int32), min_matches=0)
    assert got["best_iteration"] == -1


def test_all_samples_invalid(tv):
    c = ttv.noisy_case(65, 200)
    A, B = c["A"].copy(), c["B"].copy()
    A[:2], B[2:4] = [(2.0, 100.0), (700.0, 100.0)], [(100.0, 478.0), (100.0, 3.0)]
    samples = np.array([[0, 5, 6, 7, 8], [9, 1, 10, 11, 12], [13, 14, 2, 15, 16], [17, 18, 19, 3, 20], [0, 1, 2, 3, 30]], np.int32)
    case = small_case(A, B, samples)
    assert not case["h"].num_solutions.any() and case["res"].best_iteration == -1 and case["res"].matches == 61
    got = run_case(tv, case, "all samples invalid")
    assert not got["hyp_num_solutions"].any() and got["best_iteration"] == -1


def test_observations_at_the_roi_bounds(tv):
    """eight pairs of the noise-free scene's kind, one observation of each 0.01 px inside or outside an ROI bound"""
    c = ttv.noisy_case(65, 200)
    A, B = c["A"].copy(), c["B"].copy()
    w, h = CAM.width, CAM.height
    inside = [(4.01, 100.0), (w - 5.01, 100.0), (100.0, 4.01), (100.0, h - 5.01)]
    outside = [(3.99, 100.0), (w - 4.99, 100.0), (100.0, 3.99), (100.0, h - 4.99)]
    A[0:2], B[2:4], A[4:6], B[6:8] = inside[:2], inside[2:], outside[:2], outside[2:]
    samples = np.vstack([[[4, 10, 11, 12, 13], [14, 15, 6, 16, 17], [0, 1, 2, 3, 18]], c["samples"][:77]]).astype(np.int32)
    case = small_case(A, B, samples)
    res = case["res"]
    assert res.matches == 61 and list(case["h"].num_solutions[:2]) == [0, 0] and not set(range(4, 8)) & set(res.inliers.tolist())
    got = run_case(tv, case, "roi bounds")
    assert not set(range(4, 8)) & set(got["inliers"].tolist()) and list(got["hyp_num_solutions"][:2]) == [0, 0]


def test_point_behind_the_cameras_is_no_inlier(tv):
    """pair j's point mirrored through the first camera's centre lies behind both cameras; a pinhole projects it to the same pixel in the
    first frame and to the mirrored parallax in the last.  Its two rays meet behind the cameras: alpha, beta < 0 and d near 4"""
    c = ttv.noisy_case(65, 200)
    R, t = tm.pose_parts(tm.TRUE_POSE)
    for j in c["res"].inliers[:10].tolist():
        A, B = c["A"].copy(), c["B"].copy()
        XA = tm.triangulate_pair(R, t, tm.bearings(CAM, A[j:j + 1]), tm.bearings(CAM, B[j:j + 1]))[2][0]
        PB = R.T @ (-XA - t)
        B[j] = (CAM.fx * PB[0] / PB[2] + CAM.cx, CAM.fy * PB[1] / PB[2] + CAM.cy)
        if PB[2] >= 0 or not tm.match_mask(CAM, A[j:j + 1], B[j:j + 1])[0]:
            continue
        case = small_case(A, B, c["samples"][~(c["samples"] == j).any(axis=1)][:80], min_matches=50)
        try:
            ttv.check_case_guards(case, "behind")
        except AssertionError:
            continue
        break
    else:
        raise AssertionError("no such case found")
    assert j not in case["res"].inliers and case["res"].distances[j] > 3.0
    got = run_case(tv, case, "a point behind the cameras")
    assert j not in got["inliers"]


def test_pure_rotation_pairs_find_no_winner_or_a_sane_one(tv):
    """B = A rotated about the camera centre: every pair's rays are parallel under the true (translation-free) motion.  Whatever poses the
    samples yield, no pair may count under a pose whose rotation is that rotation, and a winner, if any, is a sane pose"""
    rng = np.random.default_rng(31)
    A = np.stack([rng.uniform(60, CAM.width - 60, 80), rng.uniform(60, CAM.height - 60, 80)], axis=1)
    R = gm.exp_se3([0, 0, 0, 0.01, -0.02, 0.015])[0]
    fb = tm.bearings(CAM, A) @ R                                          # f_A = R f_B
    B = np.stack([CAM.fx * fb[:, 0] / fb[:, 2] + CAM.cx, CAM.fy * fb[:, 1] / fb[:, 2] + CAM.cy], axis=1)
    samples = tm.draw_samples(rng, 80, 64)
    got = tv.estimate(ttv.camera_args(), A, B, samples, with_hypotheses=True)
    assert got["matches"] == 80
    used = np.arange(tm.MAX_SOLUTIONS)[None, :] < got["hyp_num_solutions"][:, None]
    assert_sane_poses(got["hyp_poses"][used], "pure rotation")
    if got["best_iteration"] >= 0:
        assert_sane_poses([got["pose_ransac"], got["pose_reselect"], got["pose"]], "pure rotation")
        assert got["inlier_count"] == len(got["inliers"]) <= 80
    # under the exact rotation with any translation the rays are parallel: d is NaN or large, never an inlier
    d = tm.distances(R, np.array([1.0, 0.0, 0.0]), tm.bearings(CAM, A), tm.bearings(CAM, B), np.ones(80, bool))
    with np.errstate(invalid="ignore"):
        assert not (d < T_ANG).any()


def test_repeated_pair_in_a_sample_is_sane(tv):
    c = ttv.noisy_case(65, 200)
    A, B = c["A"].copy(), c["B"].copy()
    A[1], B[1] = A[0], B[0]                                               # two indices, one pair of observations: the constraints have rank four
    samples = np.vstack([[[0, 1, 2, 3, 4], [5, 0, 6, 1, 7]], c["samples"][:30]]).astype(np.int32)
    got = tv.estimate(ttv.camera_args(), A, B, samples, with_hypotheses=True)
    used = np.arange(tm.MAX_SOLUTIONS)[None, :] < got["hyp_num_solutions"][:, None]
    assert ((got["hyp_num_solutions"] >= 0) & (got["hyp_num_solutions"] <= tm.MAX_SOLUTIONS)).all()
    assert_sane_poses(got["hyp_poses"][used], "a repeated pair")
    assert not got["hyp_poses"][~used].any() and not got["hyp_counts"][~used].any()
    assert_sane_poses([got["pose"]], "a repeated pair")


ERRORS = ["negative n", "negative iterations", "four pairs", "index out of range", "negative index", "repeated index", "nan observation", "inf observation",
          "nan threshold", "inf intrinsic", "null points", "null result", "null samples", "bad option", "negative min_matches"]


def test_errors_leave_the_object_usable(tv):
    from dsopp_amd import capi
    lib = capi.lib()
    c = ttv.noisy_case(65, 200)
    A, B, samples = np.array(c["A"]), np.array(c["B"]), np.array(c["samples"])
    res, idx = capi.TwoViewRansacResult(), np.zeros(len(A), np.int32)

    def call(n=len(A), iterations=len(samples), A=A, B=B, samples=samples, threshold=0.5, fx=CAM.fx, result=True, options=None, null=(), min_matches=5):
        ptr = lambda a, name, dtype=np.float64: None if name in null else capi._p(np.ascontiguousarray(a, dtype), dtype)
        return lib.dsopp_hip_two_view_ransac_estimate(tv._h, C.c_double(fx), C.c_double(CAM.fy), C.c_double(CAM.cx), C.c_double(CAM.cy), CAM.width,
                                                      CAM.height, n, ptr(A, "A"), ptr(B, "B"), iterations, ptr(samples, "samples", np.int32),
                                                      C.c_double(threshold), min_matches, C.byref(options) if options is not None else None,
                                                      C.byref(res) if result else None, capi._p(idx, np.int32), None, None, None)

    def changed(a, at, value):
        out = np.array(a)
        out[at] = value
        return out

    calls = {
        "negative n": dict(n=-1), "negative iterations": dict(iterations=-1),
        "four pairs": dict(n=4, samples=np.array([[0, 1, 2, 3, 0]], np.int32), iterations=1, min_matches=0),
        "index out of range": dict(samples=changed(samples, (3, 1), len(A))), "negative index": dict(samples=changed(samples, (0, 0), -1)),
        "repeated index": dict(samples=changed(samples, (7, 4), samples[7, 0])), "nan observation": dict(A=changed(A, (4, 1), np.nan)),
        "inf observation": dict(B=changed(B, (9, 0), np.inf)), "nan threshold": dict(threshold=np.nan), "inf intrinsic": dict(fx=np.inf),
        "null points": dict(null=("B",)), "null result": dict(result=False), "null samples": dict(null=("samples",)),
        "bad option": dict(options=capi.default_two_view_ransac_options(max_iterations=-1)), "negative min_matches": dict(min_matches=-1),
    }
    assert sorted(calls) == sorted(ERRORS)
    keep = np.zeros(len(A), np.uint8)
    for name in ERRORS:
        assert call(**calls[name]) == -1, name                              # DSOPP_HIP_ERR_INVALID_ARGUMENT
        assert lib.dsopp_hip_last_error(), name
        got = tv.estimate(ttv.camera_args(), A, B, samples)                 # and the object works as before
        assert (got["best_iteration"], got["ransac_inlier_count"]) == (c["res"].best_iteration, c["res"].ransac_inlier_count), name
    X = np.zeros((len(A), 3))
    bad = changed(tm.TRUE_POSE, 3, np.nan)
    assert lib.dsopp_hip_two_view_ransac_triangulate(tv._h, C.c_double(CAM.fx), C.c_double(CAM.fy), C.c_double(CAM.cx), C.c_double(CAM.cy), CAM.width,
                                                     CAM.height, len(A), capi._p(A), capi._p(B), capi._p(bad), capi._p(tm.IDENTITY.copy()),
                                                     C.c_double(0.9999), capi._p(X), capi._p(keep, np.uint8)) == -1
    assert tv.triangulate(ttv.camera_args(), A, B, tm.TRUE_POSE, tm.IDENTITY)[1].any()


def test_options_reach_both_refinements(tv):
    from dsopp_amd import capi
    c = ttv.noisy_case(257, 200)
    got = tv.estimate(ttv.camera_args(), c["A"], c["B"], c["samples"], options=capi.default_two_view_ransac_options(max_iterations=0))
    assert (got["refine_iterations"], got["refine_flags"]) == ((0, 0), (0, 0))
    assert np.array_equal(got["pose"], got["pose_ransac"]) and np.array_equal(got["pose_reselect"], got["pose_ransac"])
    assert got["cost_final"] == got["cost_initial"] and got["cost_initial"][0] > 0.0
    assert got["inlier_count"] == got["ransac_inlier_count"] == c["res"].ransac_inlier_count
    one = tm.estimate(CAM, c["A"], c["B"], c["samples"], max_iterations=1, hyp=c["h"])[0]
    got = tv.estimate(ttv.camera_args(), c["A"], c["B"], c["samples"], options=capi.default_two_view_ransac_options(max_iterations=1))
    assert got["refine_iterations"] == (1, 1) and np.abs(got["pose"] - one.pose).max() <= 1e-9
    wide = tm.refine(CAM, c["res"].pose_ransac, c["A"][c["res"].ransac_inliers], c["B"][c["res"].ransac_inliers], a=0.1)
    got = tv.estimate(ttv.camera_args(), c["A"], c["B"], c["samples"], options=capi.default_two_view_ransac_options(a=0.1))
    assert abs(got["cost_initial"][0] - wide.cost_initial) <= 1e-9 * wide.cost_initial                     # the Huber width too


def test_triangulate_matches_the_model(tv):
    """X within 1e-12 relative; keep exactly, outside a band of 1e-9 around each threshold; every rejection reason occurs"""
    c = ttv.noisy_case(500, 200)
    A, B = c["A"].copy(), c["B"].copy()
    A[0] = (2.0, 100.0)                                                   # outside the ROI
    B[1] = A[1]                                                           # rays parallel up to the rotation
    world = tm.pose12(gm.exp_se3([0, 0, 0, 0.1, 0.2, -0.1])[0], [1.0, 2.0, 3.0])
    flipped = tm.pose12(tm.pose_parts(c["res"].pose)[0], -c["res"].pose[9:])
    reasons = set()
    for n in (1, 255, 256, 257, 500):
        for pose in (c["res"].pose, flipped):
            X, keep = tv.triangulate(ttv.camera_args(), A[:n], B[:n], pose, world)
            Xm, km, margins = tm.triangulate(CAM, A[:n], B[:n], pose, world)
            finite = np.isfinite(Xm).all(axis=1)
            assert np.array_equal(np.isfinite(X).all(axis=1), finite)
            assert np.abs(X[finite] - Xm[finite]).max(initial=0.0) <= 1e-12 * np.abs(Xm[finite]).max(initial=1.0)
            with np.errstate(invalid="ignore"):
                clear = (np.abs(margins[:, 0]) > 1e-9) & (np.abs(margins[:, 1:] - tm.COS_THRESHOLD) > 1e-9).all(axis=1) | ~finite
                ok = tm.match_mask(CAM, A[:n], B[:n])
                reasons |= {"roi"} if (~ok).any() else set()
                reasons |= {"z"} if (ok & (margins[:, 0] <= 0)).any() else set()
                reasons |= {"cos_a"} if (ok & (margins[:, 0] > 0) & (margins[:, 1] <= tm.COS_THRESHOLD)).any() else set()
                reasons |= {"cos_b"} if (ok & (margins[:, 0] > 0) & (margins[:, 2] <= tm.COS_THRESHOLD)).any() else set()
            assert np.array_equal(keep[clear], km[clear]) and clear.sum() >= 0.99 * n
            assert keep.dtype == bool and (pose is flipped or n == 1 or keep.any())
    assert reasons == {"roi", "z", "cos_a", "cos_b"}, reasons
    X, keep = tv.triangulate(ttv.camera_args(), np.zeros((0, 2)), np.zeros((0, 2)), c["res"].pose, world)
    assert X.shape == (0, 3) and keep.shape == (0,)


# ---- the host mirror and its driver

def draw_like_the_host(libc, n, iterations, size):
    """HipEstimateSO3xS2::drawSamples (size 5) and HipRotationStandstill::drawSamples (size 3) over the C library's rand()"""
    out = np.zeros((iterations, size), np.int32)
    for i in range(iterations):
        seq = []
        while len(seq) < size:
            nxt = libc.rand() % n
            while nxt in seq:
                nxt = libc.rand() % n
            seq.append(nxt)
        out[i] = seq
    return out


def compose_like_the_host(inv, T):
    out = np.zeros(12)
    for i in range(3):
        for j in range(3):
            out[3 * i + j] = inv[3 * i] * T[j] + inv[3 * i + 1] * T[3 + j] + inv[3 * i + 2] * T[6 + j]
        out[9 + i] = inv[3 * i] * T[9] + inv[3 * i + 1] * T[10] + inv[3 * i + 2] * T[11] + inv[9 + i]
    return out


def pnp_like_the_host(pnp, libc, camera, frame, landmarks):
    fid = frame["frame_id"]
    chosen = [l for l, lm in enumerate(landmarks) if lm["has"] and fid in dict(lm["proj"])]
    X = np.array([landmarks[l]["X"] for l in chosen]).reshape(-1, 3)
    obs = np.array([dict(landmarks[l]["proj"])[fid] for l in chosen]).reshape(-1, 2)
    samples = draw_like_the_host(libc, len(chosen), 256, 3) if len(chosen) >= 3 else np.zeros((0, 3), np.int32)
    got = pnp.estimate(camera, X, obs, samples)
    frame["t_world_agent"] = gm.invert_pose(got["pose"])
    keep = {chosen[k] for k in got["inliers"]}
    for l in chosen:
        if l not in keep:
            landmarks[l]["proj"] = [(f, xy) for f, xy in landmarks[l]["proj"] if f != fid]
    return got


def test_driver_runs_the_host_mirror(tv, tmp_path):
    """example_initialize_poses.cpp drives HipInitializePoses over the C-ABI alone: the same bytes as the Python bindings composed the same
    way, over samples from the same rand() sequence"""
    import copy
    from dsopp_amd import capi
    import test_gpu_geometric_ba as tgb
    seed = 7
    track = tm.make_initialisation_track()
    cam, frames, landmarks = copy.deepcopy(track)
    camera = tuple(cam[:6])
    libc = C.CDLL("libc.so.6")
    libc.srand(seed)
    first, last = frames[0], frames[-1]
    chosen = [l for l, lm in enumerate(landmarks) if first["frame_id"] in dict(lm["proj"]) and last["frame_id"] in dict(lm["proj"])]
    A = np.array([dict(landmarks[l]["proj"])[first["frame_id"]] for l in chosen])
    B = np.array([dict(landmarks[l]["proj"])[last["frame_id"]] for l in chosen])
    two = tv.estimate(camera, A, B, draw_like_the_host(libc, len(chosen), 256, 5), options=capi.default_two_view_ransac_options(a=1.5))
    assert two["matches"] >= 50 and tm.initialised(two["inlier_count"], two["matches"]), "the track was made for an initialisation that succeeds"
    assert np.abs(two["pose"] - tm.TRUE_POSE).max() <= 2e-3
    last["t_world_agent"] = np.array(two["pose"])
    keep = {chosen[k] for k in two["inliers"]}
    for l in chosen:
        if l not in keep:
            landmarks[l]["proj"] = [(f, xy) for f, xy in landmarks[l]["proj"] if f != last["frame_id"]]
    first["initialized"] = last["initialized"] = True
    chosen = sorted(keep)
    A = np.array([dict(landmarks[l]["proj"])[first["frame_id"]] for l in chosen])
    B = np.array([dict(landmarks[l]["proj"])[last["frame_id"]] for l in chosen])
    X, kept = tv.triangulate(camera, A, B, compose_like_the_host(gm.invert_pose(first["t_world_agent"]), last["t_world_agent"]), first["t_world_agent"])
    for k, l in enumerate(chosen):
        if kept[k]:
            landmarks[l]["has"], landmarks[l]["X"] = True, X[k].copy()
    pnp = capi.PnpRansac()
    records, initialised = [], 0
    for frame in frames[1:-1]:
        got = pnp_like_the_host(pnp, libc, camera, frame, landmarks)
        records.append(got)
        if pm.initialised(got["ransac_inlier_count"], got["matches"]):
            frame["initialized"] = True
            initialised += 1
    assert initialised >= 1
    ids = [f["frame_id"] for f in frames]
    picked = [l for l, lm in enumerate(landmarks) if lm["has"] and any(fid in ids for fid, _ in lm["proj"])]
    local = [i for i, f in enumerate(frames) if f["initialized"]]
    poses, Xs, info = tgb.DeviceBackend().solve(gm._gather(cam, frames, landmarks, local, picked), 1.5)
    for f, i in enumerate(local):
        frames[i]["t_world_agent"] = gm.invert_pose(np.asarray(poses[f], np.float64))
    for k, l in enumerate(picked):
        landmarks[l]["X"] = np.array(Xs[k], np.float64)
    second = [pnp_like_the_host(pnp, libc, camera, frame, landmarks) for frame in frames[1:-1] if not frame["initialized"]]
    pnp.close()

    exe = ttv.build_example(tmp_path)
    path = str(tmp_path / "track.bin")
    tm.write_initialisation_file(path, track, seed)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().split("\n")

    def doubles(words):
        return np.array([struct.unpack("<d", struct.pack("<Q", int(w, 16)))[0] for w in words])

    def pnp_line(name, g):
        return (f"{name}: inliers {g['ransac_inlier_count']} of {g['matches']}, best {g['best_iteration']}/{g['best_solution']}, refined inliers "
                f"{g['refined_inlier_count']}, iterations {g['refine_iterations']}, flags {g['refine_flags']}")

    assert lines[0] == (f"initialised 1: two-view inliers {two['inlier_count']} of {two['matches']}, best {two['best_iteration']}/{two['best_solution']}, "
                        f"ransac inliers {two['ransac_inlier_count']}, iterations {two['refine_iterations'][0]} {two['refine_iterations'][1]}, "
                        f"flags {two['refine_flags'][0]} {two['refine_flags'][1]}, accepted 1"), lines[0]
    assert np.array_equal(doubles(lines[1].split()[2:]), two["pose"])
    assert lines[2] == f"triangulated {int(kept.sum())}, pnp initialised {initialised}", lines[2]
    at = 3
    for g in records:
        assert lines[at] == pnp_line("pnp", g), lines[at]
        at += 1
    for g in second:
        assert lines[at] == pnp_line("second pnp", g), lines[at]
        at += 1
    head = lines[at].split(", cost ")
    assert head[0] == f"refinement: iterations {info['iterations']}, accepted {info['accepted']}, reason {info['reason']}, valid {info['valid']}", lines[at]
    assert np.array_equal(doubles(head[1].split()), [info["initial_cost"], info["final_cost"]])
    words = lines[at + 1].split()[1:]
    for i, f in enumerate(frames):
        assert int(words[13 * i]) == int(f["initialized"])
        assert np.array_equal(doubles(words[13 * i + 1:13 * i + 13]), f["t_world_agent"]), i
    words = lines[at + 2].split()[1:]
    for l, lm in enumerate(landmarks):
        assert int(words[4 * l]) == int(lm["has"])
        if lm["has"]:
            assert np.array_equal(doubles(words[4 * l + 1:4 * l + 4]), lm["X"]), l
    assert [int(w) for w in lines[at + 3].split()[1:]] == [len(lm["proj"]) for lm in landmarks]
    # a file that ends early is an error, not a crash
    with open(path, "rb") as f:
        blob = f.read()
    with open(path, "wb") as f:
        f.write(blob[:len(blob) // 2])
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "too short" in r.stdout
