"""The device rotation RANSAC (dsopp_amd/csrc/rotation_ransac.hip, capi.RotationRansac) against its NumPy statement
(tests/rotation_ransac_model.py).  The bars, from include/dsopp_hip.h and DESIGN.md row i-2:
  * per-hypothesis rotations within 1e-10 entrywise, for triples whose model sigma_3 / sigma_1 >= 1e-4 (the polar factor's sensitivity is
    about eps sigma_1 / (sigma_2 + sigma_3) <= 1e-11 there);
  * per-hypothesis counts equal, leaving out every (hypothesis, point) decision whose model distance lies within 1e-6 px of the threshold
    (a 1e-10 rotation error moves a projection by less than 1e-7 px); at most 0.1 % of the decisions may be left out, and where the
    selection is compared the model must leave out none, so that the winner is determined;
  * the selection (iterations_run, best_iteration, inlier_count, the index list) exactly, the winner's rotation within 1e-10."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import rotation_ransac_model as rrm
import test_rotation_ransac as trr

pytestmark = pytest.mark.gpu

CAM = trr.CAM
THRESHOLD = 1.5
ROTATION_BAR = 1e-10
NEAR = 1e-6
MIN_SIGMA_RATIO = 1e-4


def noisy_scene(n, seed):
    """640 x 480, f = 448: A uniform in the ROI, B = A rotated by exp((0.01, -0.02, 0.005)) + N(0, 0.4 px), 30 % displaced by N(0, 15 px)"""
    rng = np.random.default_rng(seed)
    A = np.stack([rng.uniform(4.0, CAM.width - 5.0, n), rng.uniform(4.0, CAM.height - 5.0, n)], axis=1)
    B = rrm.rotate_points(CAM, trr.ROTATION, A) + rng.normal(0.0, 0.4, (n, 2))
    out = rng.random(n) < 0.3
    B[out] += rng.normal(0.0, 15.0, (int(out.sum()), 2))
    return A, B


def conditioned_triples(A, B, count, seed):
    """`count` random triples; a valid one is redrawn until the model's sigma_3 / sigma_1 >= 1e-4.  With fewer than 4 points there is one
    triple only, which is taken in random order"""
    rng = np.random.default_rng(seed)
    n, out = len(A), []
    while len(out) < count:
        s = rng.choice(n, 3, replace=False)
        valid, _, S = rrm.solve(CAM, A[s], B[s])
        if valid and S[2] / S[0] < MIN_SIGMA_RATIO and n > 3:
            continue
        out.append(s)
    return np.array(out, np.int32).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def noisy_case(n, iterations, seed=11):
    """(A, B, samples, the model's result and hypotheses), computed once per session"""
    A, B = noisy_scene(n, seed + n)
    samples = conditioned_triples(A, B, iterations, seed + 1000 + n)
    res, h = rrm.ransac(CAM, A, B, samples, THRESHOLD)
    for a in (A, B, samples):
        a.setflags(write=False)
    return A, B, samples, res, h


def camera_args():
    return (CAM.fx, CAM.fy, CAM.cx, CAM.cy, CAM.width, CAM.height)


def assert_hypotheses(got, h, threshold, pinned=None, label=""):
    """validity, rotations and counts per hypothesis; returns the number of decisions left out"""
    m = len(h.valid)
    pinned = np.ones(m, bool) if pinned is None else pinned
    assert np.array_equal(got["hyp_valid"].astype(bool), h.valid), label
    if m == 0:
        return 0
    err = np.abs(got["hyp_rotations"] - h.rotations).max(axis=(1, 2))
    print(f"{label}: greatest rotation difference {err[pinned].max() if pinned.any() else 0.0:.3e} over {int(pinned.sum())} hypotheses")
    assert (err[pinned] <= ROTATION_BAR).all(), (label, err.max(), int(np.argmax(err)))
    with np.errstate(invalid="ignore"):
        sure = (h.distances < threshold - NEAR).sum(axis=1)
        near = (np.abs(h.distances - threshold) <= NEAR).sum(axis=1)
    print(f"{label}: {int(near[pinned].sum())} of {h.distances[pinned].size} decisions within {NEAR} px of the threshold")
    dev = got["hyp_counts"].astype(np.int64)
    assert ((dev >= sure) & (dev <= sure + near))[pinned].all(), (label, dev[pinned], sure[pinned], near[pinned])
    assert near[pinned].sum() <= 1e-3 * max(h.distances[pinned].size, 1), label
    return int(near[pinned].sum())


def assert_result(got, res, label=""):
    assert got["matches"] == res.matches, label
    assert got["iterations_run"] == res.iterations_run, (label, got["iterations_run"], res.iterations_run)
    assert got["best_iteration"] == res.best_iteration, (label, got["best_iteration"], res.best_iteration)
    assert got["inlier_count"] == res.inlier_count, (label, got["inlier_count"], res.inlier_count)
    assert got["inliers"].dtype == np.int32 and np.array_equal(got["inliers"], res.inliers), label
    assert np.abs(got["rotation"] - res.rotation).max() <= ROTATION_BAR, label
    if res.best_iteration < 0:
        assert np.array_equal(got["rotation"], np.eye(3)) and len(got["inliers"]) == 0, label


def run_against_model(r, A, B, samples, threshold=THRESHOLD, tolerance=0.95, model=None, label=""):
    """the device's hypotheses and selection against the model's; the model must leave no decision out, so the winner is determined"""
    res, h = model if model is not None else rrm.ransac(CAM, A, B, samples, threshold, tolerance)
    got = r.estimate(camera_args(), A, B, samples, threshold, tolerance, with_hypotheses=True)
    if h is not None and len(samples):
        assert assert_hypotheses(got, h, threshold, label=label) == 0, f"{label}: the model leaves decisions out, the winner is not determined"
    assert_result(got, res, label)
    return got


@pytest.fixture(scope="module")
def ransac():
    from dsopp_amd import capi
    r = capi.RotationRansac()
    yield r
    r.close()


@pytest.mark.parametrize("n", [3, 4, 63, 64, 65, 257, 500, 2000])
def test_point_counts(ransac, n):
    A, B, samples, res, h = noisy_case(n, 200)
    run_against_model(ransac, A, B, samples, model=(res, h), label=f"n = {n}")


@pytest.mark.parametrize("iterations", [0, 1, 2, 200, 257])
def test_iteration_counts(ransac, iterations):
    """257: more than one workgroup, and no multiple of the hypotheses per workgroup"""
    A, B, samples, res, h = noisy_case(500, iterations)
    got = run_against_model(ransac, A, B, samples, model=(res, h), label=f"{iterations} iterations")
    if iterations == 0:
        assert got["iterations_run"] == 0 and got["best_iteration"] == -1 and got["inlier_count"] == 0


def test_every_hypothesis_is_scored_behind_an_early_stop(ransac):
    """a tolerance the first hypotheses reach: the walk stops, and the per-hypothesis outputs still cover every triple"""
    A, B, samples, _, _ = noisy_case(500, 200)
    res, h = rrm.ransac(CAM, A, B, samples, THRESHOLD, 0.5)
    assert 0 < res.iterations_run < 200
    run_against_model(ransac, A, B, samples, tolerance=0.5, model=(res, h), label="tolerance 0.5")


def outlier_scene(n=200, outliers=6):
    """clean rotated data whose first `outliers` pairs are displaced by 40 px: a triple that holds one of them is a bad hypothesis"""
    A, B = trr.clean_scene(n)
    B[:outliers] += 40.0
    return A, B


def test_early_stop_at_a_known_iteration(ransac):
    A, B = outlier_scene()
    bad = [[k % 6, 10 + k, 30 + k] for k in range(7)]
    samples = np.array(bad + [[50, 120, 180]] + [[60 + k, 90 + k, 150 + k] for k in range(12)], np.int32)
    got = run_against_model(ransac, A, B, samples, label="early stop")
    assert got["iterations_run"] == 8 and got["best_iteration"] == 7 and got["inlier_count"] == 194
    assert np.array_equal(got["inliers"], np.arange(6, 200))


def test_tie_keeps_the_earlier_hypothesis(ransac):
    A, B = outlier_scene()
    samples = np.array([[0, 10, 30], [50, 120, 180], [60, 90, 150], [70, 100, 160]], np.int32)
    got = run_against_model(ransac, A, B, samples, tolerance=2.0, label="tie")
    assert got["hyp_counts"][1] == got["hyp_counts"][2] == got["hyp_counts"][3] == 194 and got["hyp_counts"][0] < 194
    assert got["iterations_run"] == 4 and got["best_iteration"] == 1


def test_all_counts_zero(ransac):
    """a threshold no distance is below: the identity, -1 and no inliers, as the reference's default-constructed Solution"""
    A, B, samples, _, _ = noisy_case(65, 200)
    got = run_against_model(ransac, A, B, samples[:9], threshold=0.0, label="threshold 0")
    assert got["best_iteration"] == -1 and got["iterations_run"] == 9 and got["inlier_count"] == 0
    assert np.array_equal(got["rotation"], np.eye(3)) and not got["hyp_counts"].any()


def edge_scene():
    """identity data.  Pairs 0 .. 3 lie exactly on the four ROI edges, pairs 4 .. 7 one ulp outside of them, the rest well inside"""
    w, h = float(CAM.width), float(CAM.height)
    rng = np.random.default_rng(9)
    on = [[4.0, 100.0], [w - 5.0, 200.0], [300.0, 4.0], [150.0, h - 5.0]]
    off = [[np.nextafter(4.0, 0.0), 120.0], [np.nextafter(w - 5.0, 1e9), 220.0], [320.0, np.nextafter(4.0, 0.0)], [170.0, np.nextafter(h - 5.0, 1e9)]]
    inner = np.stack([rng.uniform(40, 600, 16), rng.uniform(40, 440, 16)], axis=1)
    A = np.vstack([on, off, inner])
    return A, A.copy()


def test_roi_edges(ransac):
    A, B = edge_scene()
    samples = np.array([[0, 1, 2], [1, 2, 3], [3, 0, 8]] + [[4 + k, 9, 10] for k in range(4)] + [[9, 4 + k, 11] for k in range(4)] + [[12, 13, 14]], np.int32)
    got = run_against_model(ransac, A, B, samples, tolerance=2.0, label="ROI edges")
    assert list(got["hyp_valid"]) == [1, 1, 1] + [0] * 8 + [1]
    assert (got["hyp_counts"] == 20).all()  # the identity explains every pair but the four outside
    assert np.array_equal(got["inliers"], np.r_[0:4, 8:24])
    # the same with the edge in B only: the triple is invalid, the pair is still compared
    A2 = A.copy()
    A2[4:8] += [[0.25, 0.0], [-0.25, 0.0], [0.0, 0.25], [0.0, -0.25]]  # a quarter pixel inside, B stays one ulp outside
    assert not rrm.roi(CAM, B[4:8]).any() and rrm.roi(CAM, A2).all()
    got = run_against_model(ransac, A2, B, samples, tolerance=2.0, label="ROI edges in B")
    assert list(got["hyp_valid"]) == [1, 1, 1] + [0] * 8 + [1]
    assert (got["hyp_counts"] == 24).all()


def test_invalid_triples_first(ransac):
    A, B, samples = trr.invalid_head_scene()
    got = run_against_model(ransac, A, B, samples, label="invalid head")
    assert list(got["hyp_valid"]) == [0, 0, 1, 1] and got["best_iteration"] == 0 and got["iterations_run"] == 1
    assert np.array_equal(got["hyp_rotations"][0], np.eye(3)) and np.array_equal(got["hyp_rotations"][1], np.eye(3))
    assert got["hyp_counts"][0] == got["hyp_counts"][1] == 29 and np.array_equal(got["inliers"], np.arange(1, 30))


def test_invalid_triples_after_a_valid_one(ransac):
    A, B, samples = trr.invalid_after_valid_scene()
    got = run_against_model(ransac, A, B, samples, tolerance=2.0, label="invalid after valid")
    assert list(got["hyp_valid"]) == [1, 0, 1, 0, 1]
    assert np.array_equal(got["hyp_rotations"][1], got["hyp_rotations"][0]) and got["hyp_counts"][1] == got["hyp_counts"][0]
    assert np.array_equal(got["hyp_rotations"][3], got["hyp_rotations"][2]) and got["hyp_counts"][3] == got["hyp_counts"][2]
    assert got["hyp_valid"][got["best_iteration"]] == 1


def test_invalid_triple_far_behind_its_valid_predecessor(ransac):
    """the nearest valid predecessor lies more than a wave's width of triples back"""
    A, B, _ = trr.invalid_after_valid_scene()
    samples = np.array([[0, 4, 5]] * 3 + [[1, 2, 3]] + [[0, 4 + k % 30, 39 - k % 7] for k in range(150)] + [[6, 7, 8]] + [[0, 9, 10]] * 70, np.int32)
    got = run_against_model(ransac, A, B, samples, tolerance=2.0, label="long invalid runs")
    assert got["hyp_valid"].sum() == 2 and np.array_equal(got["hyp_rotations"][153], got["hyp_rotations"][3])
    assert np.array_equal(got["hyp_rotations"][224], got["hyp_rotations"][154])


def test_points_outside_the_roi(ransac):
    A, B = trr.outside_roi_scene()
    samples = np.array([[0, 1, 2], [3, 4, 5], [23, 6, 7]], np.int32)  # the last holds the pair whose B is outside: invalid
    got = run_against_model(ransac, A, B, samples, tolerance=2.0, label="outside the ROI")
    assert list(got["hyp_valid"]) == [1, 1, 0]
    assert np.array_equal(got["inliers"], np.r_[0:20, 23]) and (got["hyp_counts"] == 21).all()


def test_singular_sample(ransac):
    """three collinear image points: sigma_3 vanishes and parity with the model is not pinned; the device must still return a rotation,
    and its count must be the model's count under the DEVICE's rotation"""
    A, B, samples, _, _ = noisy_case(257, 200)
    A, B = A.copy(), B.copy()
    A[:3] = [[100.0, 100.0], [200.0, 150.0], [300.0, 200.0]]
    B[:3] = A[:3] + [3.0, 1.5]
    assert rrm.solve(CAM, A[:3], B[:3])[2][2] < 1e-15
    samples = np.vstack([samples[:5], [[0, 1, 2]], samples[5:9]]).astype(np.int32)
    got = ransac.estimate(camera_args(), A, B, samples, THRESHOLD, 2.0, with_hypotheses=True)
    R = got["hyp_rotations"][5]
    assert got["hyp_valid"][5] == 1
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-9 and abs(np.linalg.det(R) - 1.0) <= 1e-9
    d = rrm.distances(CAM, R, A, B)
    with np.errstate(invalid="ignore"):
        sure, near = int((d < THRESHOLD - NEAR).sum()), int((np.abs(d - THRESHOLD) <= NEAR).sum())
    assert sure <= got["hyp_counts"][5] <= sure + near
    # the others are held to the model as everywhere
    _, h = rrm.ransac(CAM, A, B, samples, THRESHOLD, 2.0)
    pinned = np.ones(len(samples), bool)
    pinned[5] = False
    assert_hypotheses(got, h, THRESHOLD, pinned=pinned, label="beside a singular sample")


def test_guard_bytes_and_null_outputs(ransac):
    from dsopp_amd import capi
    A, B, samples, res, h = noisy_case(65, 200)
    n, m, guard = len(A), len(samples), 64
    sizes = {"result": C.sizeof(capi.RotationRansacResult), "indices": 4 * n, "counts": 4 * m, "rotations": 72 * m, "valid": m}
    for with_optional in (True, False):
        bufs = {k: np.full(v + guard, 0xA5, np.uint8) for k, v in sizes.items()}
        optional = [capi._p(bufs[k], np.uint8) if with_optional else None for k in ("counts", "rotations", "valid")]
        capi._chk(capi.lib().dsopp_hip_rotation_ransac_estimate(
            ransac._h, C.c_double(CAM.fx), C.c_double(CAM.fy), C.c_double(CAM.cx), C.c_double(CAM.cy), CAM.width, CAM.height, n, capi._p(A), capi._p(B), m,
            capi._p(samples, np.int32), C.c_double(THRESHOLD), C.c_double(0.95), capi._p(bufs["result"], np.uint8), capi._p(bufs["indices"], np.uint8), *optional))
        for k, v in sizes.items():
            assert np.all(bufs[k][v:] == 0xA5), k
            if not with_optional and k in ("counts", "rotations", "valid"):
                assert np.all(bufs[k] == 0xA5), k
        r = capi.RotationRansacResult.from_buffer_copy(bufs["result"][:sizes["result"]].tobytes())
        assert (r.iterations_run, r.best_iteration, r.inlier_count, r.matches) == (res.iterations_run, res.best_iteration, res.inlier_count, n)
        idx = bufs["indices"][:4 * n].view(np.int32)
        assert np.array_equal(idx[:r.inlier_count], res.inliers)
        assert np.all(bufs["indices"][4 * r.inlier_count:] == 0xA5)  # nothing behind the inliers is written
        if with_optional:
            got = {"hyp_counts": bufs["counts"][:4 * m].view(np.int32), "hyp_rotations": bufs["rotations"][:72 * m].view(np.float64).reshape(m, 3, 3),
                   "hyp_valid": bufs["valid"][:m]}
            assert_hypotheses(got, h, THRESHOLD, label="guarded outputs")


def test_repeated_and_interleaved_calls():
    """one object with growing and shrinking n and iteration counts, a second one in between"""
    from dsopp_amd import capi
    r1, r2 = capi.RotationRansac(), capi.RotationRansac()
    order = [(64, 200), (2000, 200), (3, 200), (500, 257), (65, 200), (500, 1), (2000, 200), (4, 200), (500, 200)]
    for k, (n, iterations) in enumerate(order):
        A, B, samples, res, h = noisy_case(n, iterations)
        for r in ((r1, r2) if k % 2 else (r1,)):
            run_against_model(r, A, B, samples, model=(res, h), label=f"call {k}: n = {n}, {iterations} iterations")
    r1.close()
    r2.close()


def test_small_n(ransac):
    empty = np.zeros((0, 2))
    got = ransac.estimate(camera_args(), empty, empty, np.array([[0, 1, 2]], np.int32))  # n = 0 runs no iteration, whatever the triples
    assert (got["iterations_run"], got["best_iteration"], got["inlier_count"], got["matches"]) == (0, -1, 0, 0)
    assert np.array_equal(got["rotation"], np.eye(3))
    two = np.array([[100.0, 100.0], [200.0, 200.0]])
    got = ransac.estimate(camera_args(), two, two, np.zeros((0, 3), np.int32))
    assert (got["iterations_run"], got["best_iteration"], got["inlier_count"], got["matches"]) == (0, -1, 0, 2)


def test_error_codes(ransac):
    from dsopp_amd import capi
    A, B, samples, res, h = noisy_case(64, 200)
    two = A[:2]
    for n_points in (1, 2):
        with pytest.raises(capi.HipError, match="error -1"):   # the reference's sampler never returns
            ransac.estimate(camera_args(), A[:n_points], B[:n_points], np.array([[0, 0, 0]], np.int32))
    for bad in ([0, 1, 64], [0, -1, 2], [64, 1, 2], [5, 5, 6], [5, 6, 5], [6, 5, 5]):
        s = samples.copy()
        s[137] = bad
        with pytest.raises(capi.HipError, match="error -1"):
            ransac.estimate(camera_args(), A, B, s)
    with pytest.raises(capi.HipError, match="error -1"):
        ransac.estimate(camera_args(), A, B, samples, threshold=float("nan"))
    with pytest.raises(capi.HipError, match="error -1"):
        ransac.estimate(camera_args(), A, B, samples, inliers_tolerance=float("nan"))
    result, idx = capi.RotationRansacResult(), np.zeros(64, np.int32)

    def raw(n, iterations, h=None, res=result):
        return capi.lib().dsopp_hip_rotation_ransac_estimate(
            ransac._h if h is None else h, C.c_double(CAM.fx), C.c_double(CAM.fy), C.c_double(CAM.cx), C.c_double(CAM.cy), CAM.width, CAM.height, n,
            capi._p(A), capi._p(B), iterations, capi._p(samples, np.int32), C.c_double(THRESHOLD), C.c_double(0.95),
            C.byref(res) if res is not None else None, capi._p(idx, np.int32), None, None, None)
    assert raw(64, -1) == -1 and raw(-1, 10) == -1
    assert raw(64, 10, res=None) == -1 and raw(64, 10, h=C.c_void_p()) == -1
    assert len(two) == 2 and raw(64, 10) == 0                  # and the object still works
    run_against_model(ransac, A, B, samples, model=(res, h), label="after the errors")
    with pytest.raises(capi.HipError, match="error -1"):       # no such device
        capi.RotationRansac(device=1 << 20)


def test_host_mirror_prints_the_python_result(tmp_path, ransac):
    A, B, samples, res, h = noisy_case(257, 200)
    path = tmp_path / "rotation_case.bin"
    with open(path, "wb") as f:
        f.write(b"%d %d %d %d\n" % (CAM.width, CAM.height, len(A), len(samples)))
        f.write(np.array([CAM.fx, CAM.fy, CAM.cx, CAM.cy, THRESHOLD]).tobytes() + A.tobytes() + B.tobytes() + samples.tobytes())
    exe = trr.build_example(tmp_path)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = ransac.estimate(camera_args(), A, B, samples, THRESHOLD)
    lines = r.stdout.strip().splitlines()
    assert lines[0] == "inliers %d of %d, iterations %d, best %d" % (got["inlier_count"], len(A), got["iterations_run"], got["best_iteration"])
    assert lines[1] == "rotation " + " ".join("%016x" % v for v in got["rotation"].reshape(-1).view(np.uint64))
    assert lines[2].split() == ["indices"] + [str(i) for i in got["inliers"]]
    status = rrm.need_new_frame(1, got["inlier_count"], len(A))
    assert lines[3] == "needNewFrame %s, standstill %d" % (status, rrm.is_standstill(got["inlier_count"], len(A)))
    assert_result(got, res, "the mirror's case")
    # the mirror's own triples: std::rand() from its initial state, 200 of them; the result is a plausible standstill verdict
    with open(path, "wb") as f:
        f.write(b"%d %d %d -1\n" % (CAM.width, CAM.height, len(A)))
        f.write(np.array([CAM.fx, CAM.fy, CAM.cx, CAM.cy, THRESHOLD]).tobytes() + A.tobytes() + B.tobytes())
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    head = r.stdout.splitlines()[0].replace(",", "").split()
    assert int(head[3]) == len(A) and 0.5 * len(A) < int(head[1]) <= len(A) and 1 <= int(head[5]) <= 200
