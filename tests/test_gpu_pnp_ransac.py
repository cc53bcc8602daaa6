"""The device PnP RANSAC (dsopp_amd/csrc/pnp_ransac.hip, capi.PnpRansac) against its NumPy statement (tests/pnp_ransac_model.py).  The bars,
from include/dsopp_hip.h and DESIGN.md row i-5, none of them a device result (tests/test_pnp_ransac.py computes and guards them):
  * per hypothesis: an invalid triple has no solution; on a pinned sample the number of solutions is the model's and every pose lies within
    the sample's bar, max(1e-11, 64 x the model's own change under a 1 +- 2^-52 perturbation of the triple's inputs); a sample is pinned iff
    that perturbation never changes its number of solutions and moves its poses by <= 1e-9; at most 5 % of a case's samples are unpinned;
  * counts equal, leaving out every (solution, point) decision whose model d lies within 1e-3 t_ang of t_ang (a pose error at the largest
    bar, 6.4e-8, moves d by about 1e-4 t_ang); at most 0.1 % of the decisions are left out, and no decision of a hypothesis that could
    reach the winner's count is, so the winner is determined;
  * best_iteration, best_solution and ransac_inlier_count exactly, pose_ransac within its sample's bar;
  * refine_iterations and refine_flags equal to the model's wherever the model's run takes no decision on its edge (asserted on the CPU);
    the refined pose within max(1e-11, 16 x the model's change under the same perturbation of the whole inlier set); the final inlier list
    exactly, up to points in the band.
A winner that fits exactly three points has a cost of rounding noise, and every decision of its refinement is taken on that noise: there
the record of the refinement is not compared, only what it may not break."""
import ctypes as C
import struct
import subprocess

import numpy as np
import pytest

import geometric_ba_model as gm
import pnp_ransac_model as pm
import test_pnp_ransac as tpr

pytestmark = pytest.mark.gpu

CAM = tpr.CAM
T_ANG = tpr.T_ANG


@pytest.fixture(scope="module")
def pnp():
    from dsopp_amd import capi
    r = capi.PnpRansac()
    yield r
    r.close()


def model_validity(X, obs, samples):
    return np.array([bool(pm.roi(CAM, obs[s]).all()) and not pm.triangle_is_degenerate(X[s]) for s in np.asarray(samples, np.int64).reshape(-1, 3)], bool)


def assert_hypotheses(got, c, label):
    """validity, number of solutions, poses and counts per hypothesis"""
    h, pinned, bar = c["h"], c["pinned"], c["bar"]
    m = len(c["samples"])
    num = got["hyp_num_solutions"].astype(np.int64)
    assert ((num >= 0) & (num <= 4)).all(), label
    valid = model_validity(c["X"], c["obs"], c["samples"])
    assert not num[~valid].any(), (label, "an invalid triple has solutions")
    assert np.array_equal(num[pinned], h.num_solutions[pinned]), (label, np.flatnonzero(pinned & (num != h.num_solutions)))
    unused = np.arange(4)[None, :] >= num[:, None]
    assert not got["hyp_poses"][unused].any() and not got["hyp_counts"][unused].any(), (label, "an unused slot is not zero")
    if not pinned.any():
        return
    err = np.abs(got["hyp_poses"] - h.poses).max(axis=(1, 2))
    ratio = (err / bar)[pinned]
    print(f"{label}: {int((~pinned).sum())} of {m} samples unpinned; greatest pose difference {err[pinned].max():.3e}, greatest share of a bar {ratio.max():.3f}")
    assert (ratio <= 1.0).all(), (label, int(np.argmax(np.where(pinned, err / bar, 0))), err.max())
    sure, near = c["sure"].sum(axis=2), c["near"].sum(axis=2)
    dev = got["hyp_counts"].astype(np.int64)
    assert ((dev >= sure) & (dev <= sure + near))[pinned].all(), (label, np.flatnonzero(pinned & ((dev < sure) | (dev > sure + near)).any(axis=1)))


def assert_result(got, c, label, compare_refinement=True, seed=5):
    res = c["res"]
    X, obs = c["X"], c["obs"]
    assert got["matches"] == res.matches, label
    assert (got["best_iteration"], got["best_solution"], got["ransac_inlier_count"]) == (res.best_iteration, res.best_solution, res.ransac_inlier_count), label
    if res.best_iteration < 0:
        assert np.array_equal(got["pose"], pm.IDENTITY) and np.array_equal(got["pose_ransac"], pm.IDENTITY) and len(got["inliers"]) == 0, label
        assert (got["refined_inlier_count"], got["refine_iterations"], got["refine_flags"], got["cost_initial"], got["cost_final"]) == (0, 0, 0, 0.0, 0.0), label
        return
    bar = c["bar"][res.best_iteration]
    assert np.abs(got["pose_ransac"] - res.pose_ransac).max() <= bar, label
    assert got["inliers"].dtype == np.int32 and got["refined_inlier_count"] == len(got["inliers"]), label
    assert 0 <= got["refine_iterations"] <= pm.MAX_ITERATIONS and np.isfinite(got["pose"]).all(), label
    assert got["cost_final"] <= got["cost_initial"], label
    if not compare_refinement:
        return
    assert (got["refine_iterations"], got["refine_flags"]) == (res.refine_iterations, res.refine_flags), (label, got["refine_iterations"], got["refine_flags"])
    refined_bar, change = tpr.refinement_bar(CAM, res, X, obs, seed)
    diff = np.abs(got["pose"] - res.pose).max()
    print(f"{label}: refined pose off the model by {diff:.3e}, the model's own change {change:.3e}, bar {refined_bar:.3e}")
    assert diff <= refined_bar, label
    # the start's cost moves with the start, whose distance from the model's is within `bar`: |dE| <= |b| |delta|, with |delta| <= 8 bar (12
    # entries, the scene's points within 10 m); at the end b vanishes
    _, b = pm.linearise(CAM, res.pose_ransac, X[res.ransac_inliers], obs[res.ransac_inliers])
    assert abs(got["cost_initial"] - res.cost_initial) <= 80.0 * np.linalg.norm(b) * bar + 1e-12 * res.cost_initial, label
    assert abs(got["cost_final"] - res.cost_final) <= 1e-9 * res.cost_final, label
    sure, near = tpr.near_decisions(res.distances)
    inl = set(got["inliers"].tolist())
    assert np.all(np.diff(got["inliers"]) > 0), label
    assert set(np.flatnonzero(sure).tolist()) <= inl <= set(np.flatnonzero(sure | near).tolist()), label
    assert near.sum() <= max(1e-3 * len(X), 1), label


def run_case(pnp, c, label, compare_refinement=True):
    fig = tpr.check_case_guards(c, label, compare_refinement)
    print(f"{label}: {fig}")
    got = pnp.estimate(tpr.camera_args(), c["X"], c["obs"], c["samples"], with_hypotheses=True)
    if len(c["samples"]):
        assert_hypotheses(got, c, label)
    assert_result(got, c, label, compare_refinement)
    return got


@pytest.mark.parametrize("n", [3, 4, 63, 64, 65, 257, 500, 2000])
def test_point_counts(pnp, n):
    """n = 3: one triple in its six orders, an exact fit — the refinement runs on rounding noise and its record is not compared"""
    run_case(pnp, tpr.noisy_case(n, 200), f"n = {n}", compare_refinement=n > 3)


@pytest.mark.parametrize("iterations", [0, 1, 3, 4, 5, 200, 256, 1000])
def test_hypothesis_counts(pnp, iterations):
    """the workgroup edges of four waves"""
    c = tpr.noisy_case(257, iterations)
    got = run_case(pnp, c, f"{iterations} hypotheses")
    if iterations == 0:
        assert got["best_iteration"] == -1 and got["matches"] == 257


def test_two_runs_give_the_same_bytes(pnp):
    c = tpr.noisy_case(500, 200)
    a = pnp.estimate(tpr.camera_args(), c["X"], c["obs"], c["samples"], with_hypotheses=True)
    other = tpr.noisy_case(65, 200)
    pnp.estimate(tpr.camera_args(), other["X"], other["obs"], other["samples"])          # the buffers are used in between
    b = pnp.estimate(tpr.camera_args(), c["X"], c["obs"], c["samples"], with_hypotheses=True)
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    plain = pnp.estimate(tpr.camera_args(), c["X"], c["obs"], c["samples"])
    for k in plain:
        assert np.asarray(a[k]).tobytes() == np.asarray(plain[k]).tobytes(), k


def small_case(X, obs, samples):
    X, obs, samples = np.asarray(X, np.float64), np.asarray(obs, np.float64), np.asarray(samples, np.int32).reshape(-1, 3)
    res, h = pm.estimate(CAM, X, obs, samples)
    pinned, bar, change = tpr.pin_samples(X, obs, samples, 9)
    sure, near = tpr.near_decisions(h.distances)
    return dict(X=X, obs=obs, samples=samples, res=res, h=h, pinned=pinned, bar=bar, change=change, sure=sure, near=near)


def test_all_triples_invalid(pnp):
    c = tpr.noisy_case(65, 200)
    obs = c["obs"].copy()
    obs[:3] = [(2.0, 100.0), (700.0, 100.0), (100.0, 478.0)]
    samples = np.array([[0, 5, 6], [7, 1, 8], [9, 10, 2], [0, 1, 2], [2, 20, 0]], np.int32)
    case = small_case(c["X"], obs, samples)
    assert not case["h"].num_solutions.any() and case["res"].best_iteration == -1 and case["res"].matches == 62
    got = run_case(pnp, case, "all triples invalid")
    assert not got["hyp_num_solutions"].any() and got["best_iteration"] == -1


def test_degenerate_world_triangles(pnp):
    c = tpr.noisy_case(65, 200)
    X = c["X"].copy()
    X[2] = X[0] + 2.5 * (X[1] - X[0])        # collinear
    X[5] = X[4]                              # b^2 = 0 for the triple (4, 3, 5)
    samples = np.vstack([[[0, 1, 2], [2, 0, 1], [4, 3, 5]], c["samples"][:77]]).astype(np.int32)
    case = small_case(X, c["obs"], samples)
    assert list(case["h"].num_solutions[:3]) == [0, 0, 0] and case["res"].best_iteration >= 3
    got = run_case(pnp, case, "degenerate triangles")
    assert list(got["hyp_num_solutions"][:3]) == [0, 0, 0]


def roi_edge_case():
    """eight points exactly on their rays, observed 0.01 px inside and outside each ROI bound"""
    c = tpr.noisy_case(65, 200)
    X, obs = c["X"].copy(), c["obs"].copy()
    w, h = CAM.width, CAM.height
    obs[:8] = [(4.01, 100.0), (w - 5.01, 100.0), (100.0, 4.01), (100.0, h - 5.01), (3.99, 100.0), (w - 4.99, 100.0), (100.0, 3.99), (100.0, h - 4.99)]
    R, t = pm.pose_parts(pm.TRUE_POSE)
    X[:8] = (pm.unproject(CAM, obs[:8]) * np.linspace(3.0, 9.0, 8)[:, None] - t) @ R
    samples = np.vstack([[[4, 10, 11], [12, 5, 13], [0, 1, 2], [3, 14, 15]], c["samples"][:76]]).astype(np.int32)
    return small_case(X, obs, samples)


def test_observations_at_the_roi_bounds(pnp):
    case = roi_edge_case()
    res = case["res"]
    assert res.matches == 61 and list(case["h"].num_solutions[:2]) == [0, 0] and case["h"].num_solutions[2] > 0
    assert set(range(4)) <= set(res.inliers.tolist()) and not set(range(4, 8)) & set(res.inliers.tolist())
    got = run_case(pnp, case, "roi bounds")
    assert set(range(4)) <= set(got["inliers"].tolist()) and not set(range(4, 8)) & set(got["inliers"].tolist())


def behind_case():
    """one of the scene's inliers moved along its ray to behind the camera (d = 2); the first such point whose case passes the guards"""
    c = tpr.noisy_case(65, 200)
    R, t = pm.pose_parts(pm.TRUE_POSE)
    for j in c["res"].inliers[:10].tolist():
        X = c["X"].copy()
        X[j] = (-(R @ X[j] + t) - t) @ R
        case = small_case(X, c["obs"], c["samples"][~(c["samples"] == j).any(axis=1)][:80])
        try:
            tpr.check_case_guards(case, "a point behind the camera")
        except AssertionError:
            continue
        return j, case
    raise AssertionError("no such case found")


def test_point_behind_the_camera(pnp):
    j, case = behind_case()
    assert abs(case["res"].distances[j] - 2.0) <= 1e-3 and j not in case["res"].inliers
    got = run_case(pnp, case, "a point behind the camera")
    assert j not in got["inliers"]


def no_solution_triple():
    """three matches inside the ROI whose triple has no solution in any order (found by a seeded search on the model)"""
    rng = np.random.default_rng(12)
    orders = np.array([[0, 1, 2], [0, 2, 1], [1, 0, 2], [1, 2, 0], [2, 0, 1], [2, 1, 0]], np.int32)
    for _ in range(2000):
        X = np.stack([rng.uniform(-3, 3, 3), rng.uniform(-2, 2, 3), rng.uniform(2, 10, 3)], axis=1)
        obs = np.stack([rng.uniform(8, CAM.width - 9, 3), rng.uniform(8, CAM.height - 9, 3)], axis=1)
        f = pm.bearings(CAM, obs)
        if all(len(pm.p3p(X[o], f[o])) == 0 for o in orders) and not pm.triangle_is_degenerate(X):
            return X, obs, orders
    raise AssertionError("no triple without a solution found")


def test_all_matches_outliers(pnp):
    """valid triples, none of which has a pose: every count is 0, best_iteration = -1, the identity, no refinement"""
    X, obs, orders = no_solution_triple()
    case = small_case(X, obs, orders)
    assert case["res"].best_iteration == -1 and case["res"].matches == 3 and case["pinned"].all()
    got = run_case(pnp, case, "all matches outliers")
    assert not got["hyp_counts"].any() and got["best_iteration"] == -1 and np.array_equal(got["pose"], pm.IDENTITY)


def test_no_points(pnp):
    got = pnp.estimate(tpr.camera_args(), np.zeros((0, 3)), np.zeros((0, 2)), np.zeros((0, 3), np.int32), with_hypotheses=True)
    assert (got["matches"], got["best_iteration"], got["best_solution"], got["ransac_inlier_count"], got["refined_inlier_count"]) == (0, -1, -1, 0, 0)
    assert np.array_equal(got["pose"], pm.IDENTITY) and len(got["inliers"]) == 0
    # triples are not looked at without points
    got = pnp.estimate(tpr.camera_args(), np.zeros((0, 3)), np.zeros((0, 2)), np.array([[0, 1, 2]], np.int32))
    assert got["best_iteration"] == -1


def test_winner_with_exactly_three_inliers(pnp):
    """random observations: a triple explains itself and nothing else.  The cost is rounding noise, the 6 x 6 system of three points is
    barely regular and its Cholesky may fail (the iteration then counts as rejected): the refinement's record is not compared, but the pose
    it leaves must still explain the three points"""
    rng = np.random.default_rng(21)
    for _ in range(50):
        X = np.stack([rng.uniform(-3, 3, 12), rng.uniform(-2, 2, 12), rng.uniform(2, 10, 12)], axis=1)
        obs = np.stack([rng.uniform(8, CAM.width - 9, 12), rng.uniform(8, CAM.height - 9, 12)], axis=1)
        case = small_case(X, obs, pm.draw_triples(rng, 12, 9))
        if case["res"].ransac_inlier_count == 3 and case["pinned"].all() and not case["near"].any():
            break
    else:
        raise AssertionError("no such scene found")
    res = case["res"]
    got = run_case(pnp, case, "three inliers", compare_refinement=False)
    assert got["ransac_inlier_count"] == 3 and list(got["inliers"]) == list(res.ransac_inliers) == list(res.inliers)


ERRORS = ["negative n", "negative iterations", "two points", "index out of range", "negative index", "repeated index", "nan position", "inf observation",
          "nan threshold", "inf intrinsic", "null positions", "null result", "null samples", "bad option"]


def test_errors_leave_the_object_usable(pnp):
    from dsopp_amd import capi
    lib = capi.lib()
    c = tpr.noisy_case(65, 200)
    X, obs, samples = np.array(c["X"]), np.array(c["obs"]), np.array(c["samples"])
    res, idx = capi.PnpRansacResult(), np.zeros(len(X), np.int32)

    def call(n=len(X), iterations=len(samples), X=X, obs=obs, samples=samples, threshold=0.5, fx=CAM.fx, result=True, options=None, null=()):
        ptr = lambda a, name, dtype=np.float64: None if name in null else capi._p(np.ascontiguousarray(a, dtype), dtype)
        return lib.dsopp_hip_pnp_ransac_estimate(pnp._h, C.c_double(fx), C.c_double(CAM.fy), C.c_double(CAM.cx), C.c_double(CAM.cy), CAM.width, CAM.height,
                                                 n, ptr(X, "X"), ptr(obs, "obs"), iterations, ptr(samples, "samples", np.int32), C.c_double(threshold),
                                                 C.byref(options) if options is not None else None, C.byref(res) if result else None,
                                                 capi._p(idx, np.int32), None, None, None)

    def changed(a, at, value):
        out = np.array(a)
        out[at] = value
        return out

    calls = {
        "negative n": dict(n=-1), "negative iterations": dict(iterations=-1), "two points": dict(n=2, samples=np.array([[0, 1, 0]], np.int32), iterations=1),
        "index out of range": dict(samples=changed(samples, (3, 1), len(X))), "negative index": dict(samples=changed(samples, (0, 0), -1)),
        "repeated index": dict(samples=changed(samples, (7, 2), samples[7, 0])), "nan position": dict(X=changed(X, (4, 1), np.nan)),
        "inf observation": dict(obs=changed(obs, (9, 0), np.inf)), "nan threshold": dict(threshold=np.nan), "inf intrinsic": dict(fx=np.inf),
        "null positions": dict(null=("X",)), "null result": dict(result=False), "null samples": dict(null=("samples",)),
        "bad option": dict(options=capi.default_pnp_ransac_options(max_iterations=-1)),
    }
    assert sorted(calls) == sorted(ERRORS)
    for name in ERRORS:
        assert call(**calls[name]) == -1, name                              # DSOPP_HIP_ERR_INVALID_ARGUMENT
        assert lib.dsopp_hip_last_error(), name
        got = pnp.estimate(tpr.camera_args(), X, obs, samples)              # and the object works as before
        assert (got["best_iteration"], got["ransac_inlier_count"]) == (c["res"].best_iteration, c["res"].ransac_inlier_count), name


def test_options_reach_the_refinement(pnp):
    from dsopp_amd import capi
    c = tpr.noisy_case(257, 200)
    got = pnp.estimate(tpr.camera_args(), c["X"], c["obs"], c["samples"], options=capi.default_pnp_ransac_options(max_iterations=0))
    assert (got["refine_iterations"], got["refine_flags"]) == (0, 0) and np.array_equal(got["pose"], got["pose_ransac"])
    assert got["cost_final"] == got["cost_initial"] > 0.0
    one = pm.estimate(CAM, c["X"], c["obs"], c["samples"], max_iterations=1, hyp=c["h"])[0]
    got = pnp.estimate(tpr.camera_args(), c["X"], c["obs"], c["samples"], options=capi.default_pnp_ransac_options(max_iterations=1))
    assert got["refine_iterations"] == 1 and np.abs(got["pose"] - one.pose).max() <= 1e-9


# ---- the host mirror and its driver

def make_track(F=6, L=150, seed=71):
    """geometric_ba_model.make_track with landmark positions a PnP can use: frames = dicts frame_id, t_world_agent, initialized; landmarks =
    dicts has, X, proj.  Half of the landmarks carry a position a few millimetres off the truth."""
    truth, rng = gm.make_scene(F=F, L=L, seed=seed, noise=0.2)
    start = gm.perturb(truth, rng, pose_sigma=0.002, point_sigma=0.002)
    frames = [dict(frame_id=10 + 3 * f, t_world_agent=gm.invert_pose(start.poses[f]), initialized=True) for f in range(F)]
    landmarks = []
    for l in range(L):
        o = range(truth.off[l], truth.off[l + 1])
        landmarks.append(dict(has=bool(rng.uniform() < 0.5), X=start.X[l].copy(), proj=[(frames[truth.ofr[k]]["frame_id"], truth.oxy[k].copy()) for k in o]))
    return truth.cam, frames, landmarks


def draw_samples_like_the_host(libc, n, iterations):
    """HipRotationStandstill::drawSamples over the C library's rand()"""
    out = np.zeros((iterations, 3), np.int32)
    for i in range(iterations):
        seq = [libc.rand() % n]
        while len(seq) < 3:
            nxt = libc.rand() % n
            while nxt in seq:
                nxt = libc.rand() % n
            seq.append(nxt)
        out[i] = seq
    return out


def test_driver_runs_the_host_mirror(pnp, tmp_path):
    """example_bootstrap_frame.cpp drives HipEstimateSE3PnP and HipRefineTrack over the C-ABI alone: the same bytes as the Python bindings
    composed the same way, over triples from the same rand() sequence"""
    import copy
    import test_gpu_geometric_ba as tgb
    steps = 2
    track = make_track()
    cam, frames, landmarks = copy.deepcopy(track)
    camera = (cam[0], cam[1], cam[2], cam[3], cam[4], cam[5])
    libc = C.CDLL("libc.so.6")
    expected = []
    for step in range(steps):
        present = frames[:len(frames) - steps + step + 1]
        frame = present[-1]
        fid = frame["frame_id"]
        chosen = [l for l, lm in enumerate(landmarks) if lm["has"] and fid in dict(lm["proj"])]
        X = np.array([landmarks[l]["X"] for l in chosen]).reshape(-1, 3)
        obs = np.array([dict(landmarks[l]["proj"])[fid] for l in chosen]).reshape(-1, 2)
        libc.srand(step + 1)                                                # as the driver seeds each step
        samples = draw_samples_like_the_host(libc, len(chosen), 256)
        got = pnp.estimate(camera, X, obs, samples)
        assert got["ransac_inlier_count"] > 0.5 * got["matches"] > 10, "the track was made for a PnP that succeeds"
        frame["t_world_agent"] = gm.invert_pose(got["pose"])
        frame["initialized"] = True
        keep = {chosen[k] for k in got["inliers"]}
        for l in chosen:
            if l not in keep:
                landmarks[l]["proj"] = [(f, xy) for f, xy in landmarks[l]["proj"] if f != fid]
        rec = gm.bootstrap_frame(tgb.DeviceBackend(), cam, present, landmarks)
        expected.append((got, rec, [np.array(f["t_world_agent"]) for f in present]))
    exe = tpr.build_example(tmp_path)
    path = str(tmp_path / "track.bin")
    gm.write_track_file(path, track, steps)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 7 * steps, r.stdout

    def doubles(words):
        return np.array([struct.unpack("<d", struct.pack("<Q", int(w, 16)))[0] for w in words])

    for step, (got, rec, poses) in enumerate(expected):
        block = lines[7 * step:7 * step + 7]
        assert block[0] == (f"step {step}: pnp inliers {got['ransac_inlier_count']} of {got['matches']}, best {got['best_iteration']}/{got['best_solution']}, "
                            f"refined inliers {got['refined_inlier_count']}, iterations {got['refine_iterations']}, flags {got['refine_flags']}, "
                            f"initialised {int(pm.initialised(got['ransac_inlier_count'], got['matches']))}"), block[0]
        assert np.array_equal(doubles(block[1].split()[2:]), got["pose"])
        assert block[2] == (f"step {step}: triangulated {rec['triangulated']}, iterations {rec['iterations']}, accepted {rec['accepted']}, "
                            f"reason {rec['reason']}, valid {rec['valid']}, removed {rec['removed']}"), block[2]
        assert np.array_equal(doubles(block[3].split()[1:]), [rec["initial_cost"], rec["final_cost"]])
        assert np.array_equal(doubles(block[4].split()[1:]).reshape(-1, 12), np.array(poses))
    words = lines[-2].split()[1:]
    for l, lm in enumerate(landmarks):
        assert int(words[4 * l]) == int(lm["has"])
        if lm["has"]:
            assert np.array_equal(doubles(words[4 * l + 1:4 * l + 4]), lm["X"]), l
    assert [int(w) for w in lines[-1].split()[1:]] == [len(lm["proj"]) for lm in landmarks]
    # a file that ends early is an error, not a crash
    with open(path, "rb") as f:
        blob = f.read()
    with open(path, "wb") as f:
        f.write(blob[:len(blob) // 2])
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "too short" in r.stdout
