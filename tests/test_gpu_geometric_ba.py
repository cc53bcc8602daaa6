"""The device geometric bundle adjustment (dsopp_amd/csrc/geometric_ba.hip, capi.GeometricBA) against its NumPy statement
(tests/geometric_ba_model.py).  The bars, from include/dsopp_hip.h and DESIGN.md row i-4:
  evaluate      validity equal (no decision of these scenes lies within 1e-9 px or depth of a threshold: asserted on the model), residuals
                within 1e-9 px, cost within 1e-10 relative
  linearise     landmark blocks, reduced system and right-hand sides within 1e-9 of sqrt(H_ii H_jj) and of sqrt(H_ii sum w r^2), the
                Cauchy-Schwarz bound of a right-hand side's entry
  step          the componentwise backward error of the device's pose step against the system the device hands out, in extended
                precision, within 16 max(omega_lapack, u) (tests/dense_solve_model.py's factor); the rest of the iteration against the model
                applied to the device's own step at 1e-12 relative (positions to 1 + |X|, the candidate's cost to the cost before)
  one iteration from the model's states: accept flag and new lambda equal
  full solve    final state within 16 max(d, 1e-12) of the float64 model's, d = the distance of the float64 and the longdouble model runs;
                iteration count and accept pattern equal
  triangulation flags equal; positions within 1e-9 * 2 (1 + |X|^2) where (l3 - l4) / l1 >= 1e-6, finite elsewhere
  pruning       flags equal."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_solve_model as dsm
import geometric_ba_model as gm
from dsopp_amd import capi

pytestmark = pytest.mark.gpu

def args(pr):
    return pr.cam, np.asarray(pr.poses, np.float64), np.asarray(pr.X, np.float64), pr.off, pr.ofr, pr.oxy


@functools.lru_cache(maxsize=None)
def ba():
    return capi.GeometricBA()


# (F, L, seed, noise, outliers): F = 2 leaves only the five-DoF frame free; L = 63, 64, 65 straddle a wavefront, 300 and 3000 more than
# one workgroup per stage; landmarks carry 1 .. F observations
SCENES = {"F2_L1": (2, 1, 50, 0.3, 0.0), "F2_L40": (2, 40, 3, 0.3, 0.0), "F3_L63": (3, 63, 4, 0.3, 0.0), "F10_L64": (10, 64, 5, 0.3, 0.0),
          "F16_L65": (16, 65, 6, 0.3, 0.0), "F5_L300": (5, 300, 7, 0.3, 0.0), "F10_L3000": (10, 3000, 8, 0.3, 0.0),
          "F5_L120_outliers": (5, 120, 22, 0.3, 0.3)}


@functools.lru_cache(maxsize=None)
def scene(name):
    F, L, seed, noise, outliers = SCENES[name]
    truth, rng = gm.make_scene(F=F, L=L, seed=seed, noise=noise, outliers=outliers)
    return truth, gm.perturb(truth, rng)


@functools.lru_cache(maxsize=None)
def one_observation_scene():
    """F = 4, landmarks with 1, 2 and F observations side by side"""
    truth, rng = gm.make_scene(F=4, L=90, seed=60, noise=0.3, min_obs=1)
    counts = np.diff(truth.off)
    assert {1, 2, 4} <= set(counts.tolist())
    return truth, gm.perturb(truth, rng)


def assert_no_near_decision(pr):
    depth, edge = gm.decision_margins(pr)
    assert depth.min() > 1e-9 and edge.min() > 1e-9, (depth.min(), edge.min())


# ---- evaluate

@pytest.mark.parametrize("name", list(SCENES) + ["one_observation"])
def test_evaluate(name):
    pr = one_observation_scene()[1] if name == "one_observation" else scene(name)[1]
    assert_no_near_decision(pr)
    ev = gm.evaluate(pr)
    out = ba().evaluate(*args(pr), with_observations=True)
    assert np.array_equal(out["obs_valid"].astype(bool), ev["valid"])
    assert out["valid_residuals"] == ev["nvalid"]
    err = np.abs(out["obs_residual"] - ev["r"]).max()
    rel = abs(out["cost"] - ev["cost"]) / ev["cost"]
    print(f"{name}: residual error {err:.3e} px, cost relative error {rel:.3e}")
    assert err <= 1e-9
    assert rel <= 1e-10
    assert np.abs(out["obs_weight"] - ev["w"]).max() <= 1e-12


def edge_problem():
    """Frame 0 is the identity and the camera's constants are powers of two, so q of the hand-made points is exact on the device and in the
    model alike: decisions AT a threshold are compared, not left out.  Landmark 0: q_x exactly 4 (inside); 1: one ulp of the product
    outside; 2: one ulp inside; 3: behind the camera in frame 0 and in frame 1 (all observations invalid); 4: p_z just below 0.001 in frame
    0, fine in frame 1; 5: |r| exactly a; 6: |r| = a + 2^-30; 7: an ordinary point."""
    cam = (256.0, 256.0, 128.0, 128.0, 256, 256)
    poses = np.zeros((2, 12))
    poses[:, [0, 4, 8]] = 1.0
    poses[1, 9:] = [0.25, 0.0, 0.5]
    px = (4.0 - 128.0) / 256.0
    X = np.array([[px, 0.0, 1.0], [np.nextafter(px, -1.0), 0.0, 1.0], [np.nextafter(px, 0.0), 0.0, 1.0], [0.1, 0.1, -2.0],
                  [-0.1, 0.0, 0.0009], [0.125, 0.125, 1.0], [0.125, -0.125, 1.0], [0.2, 0.1, 2.0]])
    off = np.arange(0, 17, 2)
    ofr = np.tile([0, 1], 8)
    pr = gm.Problem(cam, poses, X, off, ofr, np.zeros((16, 2)))
    _, q, _ = gm.project(pr)
    oxy = q + 0.25
    oxy[10] = q[10] + [1.5, 0.0]
    oxy[12] = q[12] + [1.5 + 2.0 ** -30, 0.0]
    return gm.Problem(cam, poses, X, off, ofr, oxy)


def test_evaluate_at_the_thresholds():
    pr = edge_problem()
    ev = gm.evaluate(pr)
    # the model itself decides as designed
    assert ev["valid"].tolist() == [True, True, False, True, True, True, False, False, False, True] + [True] * 6
    assert np.all(ev["r"][10] == [1.5, 0.0]) and np.all(ev["r"][12] == [1.5 + 2.0 ** -30, 0.0])
    assert ev["w"][10] == 1.0 and 0.0 < ev["w"][12] < 1.0
    out = ba().evaluate(*args(pr), with_observations=True)
    assert np.array_equal(out["obs_valid"].astype(bool), ev["valid"])
    assert np.abs(out["obs_residual"] - ev["r"]).max() <= 1e-9
    assert out["obs_weight"][10] == 1.0 and 0.0 < out["obs_weight"][12] < 1.0
    assert np.all(out["obs_residual"][~ev["valid"]] == 0.0) and np.all(out["obs_weight"][~ev["valid"]] == 0.0)
    assert abs(out["cost"] - ev["cost"]) <= 1e-10 * ev["cost"]


# ---- one iteration: the linearisation, the step, the rest

def packed_blocks(Hll):
    return np.stack([Hll[:, 0, 0], Hll[:, 0, 1], Hll[:, 0, 2], Hll[:, 1, 1], Hll[:, 1, 2], Hll[:, 2, 2]], -1)


def backward_error(H, g, x):
    """omega = max_i |H x - g|_i / (sqrt(H_ii) sum_j sqrt(H_jj) |x_j| + |g_i|), in extended precision (tests/dense_solve_model.py's measure
    for a system that is handed out assembled)"""
    B = dsm.backend()
    Hx, gx, xx = B.arr(H), B.arr(g), B.arr(x)
    r = Hx @ xx - gx
    rs = B.sqrt(np.abs(np.diagonal(Hx).copy()))
    den = rs * (rs @ np.abs(xx)) + np.abs(gx)
    return max(float(abs(r[i]) / den[i]) for i in range(len(g)))


ITERATION_SCENES = ["F2_L1", "F2_L40", "F3_L63", "F10_L64", "F16_L65", "F5_L300", "F10_L3000", "F5_L120_outliers", "one_observation",
                    "thresholds"]


@pytest.mark.parametrize("name", ITERATION_SCENES)
def test_one_iteration(name):
    from scipy.linalg import cho_factor, cho_solve
    pr = {"one_observation": lambda: one_observation_scene()[1], "thresholds": edge_problem}.get(name, lambda: scene(name)[1])()
    lam = gm.LAMBDA_0
    norm1 = np.linalg.norm(pr.poses[1, 9:])
    lin = gm.linearise(pr)
    H, g, extra = gm.reduced_system(pr, lin, lam, norm1)
    out = ba().solve(*args(pr), debug=True, max_iterations=1)
    assert out["iterations"] == 1 and out["system_lambda"] == lam
    # the linearisation
    assert np.array_equal(out["obs_valid"].astype(bool), lin["valid"])
    d = np.sqrt(np.abs(np.stack([lin["Hll"][:, i, i] for i in range(3)], -1)))
    scale = packed_blocks(d[:, :, None] * d[:, None, :])
    eH = np.abs(out["landmark_H"] - packed_blocks(lin["Hll"]))
    assert np.all(eH <= 1e-9 * scale), (eH / np.maximum(scale, 1e-300)).max()
    wr2 = np.zeros(pr.L)
    np.add.at(wr2, pr.obl, lin["w"] * np.sum(lin["r"] ** 2, -1))
    eb = np.abs(out["landmark_b"] - lin["bl"])
    assert np.all(eb <= 1e-9 * d * np.sqrt(wr2)[:, None])
    dp = np.sqrt(np.diag(extra["Hm"]))                      # the undamped pose diagonal: what was added into every entry
    eS = np.abs(out["reduced_H"] - H)
    eg = np.abs(out["reduced_b"] - g)
    print(f"{name}: reduced system error {(eS / np.outer(dp, dp)).max():.3e}, right-hand side {(eg / (dp * np.sqrt(wr2.sum()))).max():.3e}")
    assert np.all(eS <= 1e-9 * np.outer(dp, dp))
    assert np.all(eg <= 1e-9 * dp * np.sqrt(wr2.sum()))
    # the step: backward error against the device's own system
    x = out["pose_step"]
    assert np.all(np.isfinite(x))
    omega = backward_error(out["reduced_H"], out["reduced_b"], x)
    omega_lapack = backward_error(out["reduced_H"], out["reduced_b"], cho_solve(cho_factor(out["reduced_H"], lower=True), out["reduced_b"]))
    print(f"{name}: omega {omega:.3e}, omega_lapack {omega_lapack:.3e}")
    assert omega <= dsm.working_threshold(omega_lapack), (omega, omega_lapack)
    # the rest of the iteration, from the device's own step
    st = gm.apply_step(pr, lin, lam, norm1, x)
    cand = st["candidate"]
    ep = np.abs(out["candidate_poses"] - cand.poses).max()
    ex = (np.abs(out["candidate_positions"] - cand.X) / (1.0 + np.abs(cand.X))).max()
    cost_before, cost_candidate, accepted, lam_used = out["trace"][0]
    # the candidate's cost relative to the cost it is compared with, the driver's own normalisation |E - E'| / E: a candidate that fits
    # almost exactly (F = 2 with one landmark) has a cost that is all cancellation, and no relative figure of its own
    ec = abs(cost_candidate - st["cost"]) / cost_before
    print(f"{name}: candidate poses {ep:.3e}, positions {ex:.3e} relative, cost {ec:.3e} of the cost before")
    assert ep <= 1e-12 and ex <= 1e-12 and ec <= 1e-12
    assert lam_used == lam and abs(cost_before - lin["cost"]) <= 1e-10 * lin["cost"]


# ---- one iteration from each of the model's states

@functools.lru_cache(maxsize=None)
def model_run(name):
    if name == "rejected_first":
        # the state the outlier run reaches after its first step: the next three steps are rejected
        base, _ = model_run("F5_L120_outliers")
        start, lam = base["states"][1]
        run = gm.solve(start, lambda_0=float(lam), keep_states=True)
        assert [t[2] for t in run["trace"]][:3] == [0, 0, 0]
        return run, gm.FTOL
    # without outliers the last iterations of a run at the reference's tolerance change the cost by less than 1e-6 of itself: those runs
    # end at a function tolerance of 1e-5 instead, so that only the closing iteration can lie near a decision
    ftol = gm.FTOL if "outliers" in name else 1e-5
    return gm.solve(scene(name)[1], ftol=ftol, keep_states=True), ftol


@pytest.mark.parametrize("name", ["F3_L63", "F10_L64", "F5_L120_outliers", "rejected_first"])
def test_one_iteration_from_the_models_states(name):
    run, ftol = model_run(name)
    left_out = 0
    for k, ((state, lam), (E, En, accepted, _)) in enumerate(zip(run["states"], run["trace"])):
        rel = abs(float(E - En)) / float(E)
        if rel < 1e-6 or abs(rel - ftol) < 1e-6:     # a decision within 1e-6 (relative cost change) of flipping
            left_out += 1
            continue
        out = ba().solve(*args(state), lambda_0=float(lam), function_tolerance=ftol, max_iterations=1)
        assert bool(out["reason"] & gm.FUNCTION_TOLERANCE) == (rel < ftol), (name, k, out["reason"], rel)
        lam_next = float(lam) / gm.DECREASE if accepted else float(lam) * gm.INCREASE
        assert (out["accepted_steps"], out["final_lambda"]) == (accepted, lam_next), (name, k, out, accepted, lam_next)
    # by construction only a run's closing iteration (the one that meets the function tolerance) can be near
    assert left_out <= 1, left_out


# ---- the full solve

@functools.lru_cache(maxsize=None)
def model_pair(name, max_iterations):
    start = scene(name)[1]
    a = gm.solve(start, max_iterations=max_iterations)
    b = gm.solve(start, max_iterations=max_iterations, dtype=np.longdouble)
    pattern = [t[2] for t in a["trace"]]
    assert a["iterations"] == b["iterations"] and pattern == [t[2] for t in b["trace"]], "the seed was chosen so that the model runs agree"
    d = max(float(np.abs(a["problem"].poses - b["problem"].poses).max()), float(np.abs(a["problem"].X - b["problem"].X).max()))
    return a, pattern, d


@pytest.mark.parametrize("name,max_iterations", [("F2_L40", 50), ("F3_L63", 50), ("F10_L64", 50), ("F16_L65", 50), ("F5_L300", 50),
                                                 ("F10_L3000", 8), ("F5_L120_outliers", 50)])
def test_full_solve(name, max_iterations):
    a, pattern, d = model_pair(name, max_iterations)
    out = ba().solve(*args(scene(name)[1]), debug=True, max_iterations=max_iterations)
    dist = max(np.abs(out["poses"] - a["problem"].poses).max(), np.abs(out["positions"] - a["problem"].X).max())
    print(f"{name}: {out['iterations']} iterations, d = {d:.3e}, device distance {dist:.3e}, bar {16 * max(d, 1e-12):.3e}")
    assert out["iterations"] == a["iterations"] and [t[2] for t in out["trace"]] == pattern
    assert out["reason"] == a["reason"] and out["converged"] == int(a["converged"]) and out["accepted_steps"] == a["accepted"]
    assert dist <= 16 * max(d, 1e-12)
    assert abs(out["final_cost"] - a["final_cost"]) <= 1e-9 * a["final_cost"] and out["valid_residuals"] == a["nvalid"]
    assert abs(out["initial_cost"] - a["initial_cost"]) <= 1e-10 * a["initial_cost"]
    assert out["final_lambda"] == float(a["lambda"])


def test_iteration_group_does_not_change_the_result():
    start = scene("F5_L120_outliers")[1]
    base = ba().solve(*args(start), iteration_group=1)
    for group in (3, 64):
        other = ba().solve(*args(start), iteration_group=group)
        assert other["poses"].tobytes() == base["poses"].tobytes() and other["positions"].tobytes() == base["positions"].tobytes()
        assert (other["iterations"], other["final_cost"]) == (base["iterations"], base["final_cost"])


# ---- triangulation and pruning

@pytest.mark.parametrize("name", ["F10_L64", "F16_L65", "F10_L3000"])
def test_triangulation(name):
    truth, start = scene(name)
    rng = np.random.default_rng(1)
    has = (rng.uniform(size=truth.L) < 0.3).astype(np.uint8)
    counts = np.diff(truth.off)
    assert (counts == 4).any() and (counts == 5).any(), "exactly min_number_of_projections and one more are both present"
    given = np.where(has[:, None].astype(bool), start.X, np.nan)          # a landmark without a position carries none
    pr = truth.with_state(truth.poses, given)
    for retriangulation in (False, True):
        run, X, vals = gm.triangulate(pr, has, 4, retriangulation)
        done, Xd = ba().triangulate(*args(pr), has, 4, retriangulation)
        assert np.array_equal(done.astype(bool), run)
        assert not run[counts <= 4].any() and (retriangulation or not run[has.astype(bool)].any())
        same = ~run
        assert np.array_equal(Xd[same], given[same], equal_nan=True)
        assert np.all(np.isfinite(Xd[run]))
        pinned = run & ((vals[:, 1] - vals[:, 0]) / vals[:, 3] >= 1e-6)
        assert pinned.sum() >= 0.9 * run.sum()
        bar = 1e-9 * 2 * (1 + np.sum(X[pinned] ** 2, -1))
        err = np.abs(Xd[pinned] - X[pinned]).max(-1)
        print(f"{name} retriangulation={retriangulation}: {int(run.sum())} triangulated, worst error / bar {(err / bar).max():.3e}")
        assert np.all(err <= bar)


@pytest.mark.parametrize("name", ["F2_L1", "F3_L63", "F10_L3000", "F5_L120_outliers", "thresholds"])
def test_pruning(name):
    if name == "thresholds":
        pr = edge_problem()         # exact projections: decisions at the ROI's edge are compared too
    else:
        pr = scene(name)[0]          # the truth: noisy observations scatter around the 0.5 px threshold
        assert_no_near_decision(pr)
    flags = gm.flag_outliers(pr)
    _, q, _ = gm.project(pr)
    dist = np.sqrt(np.sum((pr.oxy - q) ** 2, -1))
    assert name == "thresholds" or np.abs(dist - 0.5).min() > 1e-9
    out = ba().flag_outliers(*args(pr))
    assert np.array_equal(out.astype(bool), flags)
    assert name in ("F2_L1", "thresholds") or 0 < flags.sum() < pr.M


# ---- plumbing

def test_repeated_and_interleaved_calls_return_identical_bytes():
    a, b = capi.GeometricBA(), capi.GeometricBA()
    p1, p2 = scene("F5_L300")[1], scene("F10_L64")[1]
    keys = ("poses", "positions", "reduced_H", "reduced_b", "pose_step", "landmark_H", "candidate_positions", "obs_residual")
    first = {}
    for rnd in range(3):
        for obj, pr, tag in ((a, p1, "a1"), (b, p2, "b2"), (a, p2, "a2"), (b, p1, "b1")):
            out = obj.solve(*args(pr), debug=True)
            blob = b"".join(out[k].tobytes() for k in keys) + repr((out["trace"], out["iterations"], out["final_cost"])).encode()
            assert first.setdefault(tag[1], blob) == blob, (rnd, tag)
            ev = obj.evaluate(*args(pr), with_observations=True)
            assert first.setdefault("e" + tag[1], ev["obs_residual"].tobytes() + repr(ev["cost"]).encode()) == ev["obs_residual"].tobytes() + repr(ev["cost"]).encode()
    a.close()
    b.close()


def guarded(nbytes):
    buf = np.full(nbytes + 128, 0xA5, np.uint8)
    return buf, buf[64:64 + nbytes]


def test_guard_bytes_around_every_output():
    pr = scene("F3_L63")[1]
    problem, keep = capi.GeometricBA.problem(*args(pr))
    F, L, M = pr.F, pr.L, pr.M
    n = 6 * (F - 1) - 1
    iters = 5
    sizes = dict(obs_valid=M, obs_residual=16 * M, obs_weight=8 * M, landmark_H=48 * L, landmark_b=24 * L, reduced_H=8 * n * n, reduced_b=8 * n,
                 pose_step=8 * n, system_lambda=8, candidate_poses=96 * F, candidate_positions=24 * L,
                 trace=iters * C.sizeof(capi.GeometricBATrace))
    bufs = {k: guarded(v) for k, v in sizes.items()}
    bufs.update(poses=guarded(96 * F), positions=guarded(24 * L), result=guarded(C.sizeof(capi.GeometricBAResult)), flags=guarded(M),
                triangulated=guarded(L), e_valid=guarded(M), e_res=guarded(16 * M), e_w=guarded(8 * M))
    bufs["poses"][1][:] = keep[0].view(np.uint8).reshape(-1)
    bufs["positions"][1][:] = keep[1].view(np.uint8).reshape(-1)
    problem.poses, problem.positions = bufs["poses"][1].ctypes.data, bufs["positions"][1].ctypes.data
    dbg = capi.GeometricBADebug(*[bufs[name][1].ctypes.data for name in capi.GEOMETRIC_BA_DEBUG_FIELDS])
    opt = capi.default_geometric_ba_options(max_iterations=iters)
    h = ba()._h
    lib = capi.lib()
    capi._chk(lib.dsopp_hip_geometric_ba_solve(h, C.byref(problem), C.byref(opt), C.c_void_p(bufs["result"][1].ctypes.data), C.byref(dbg)))
    res = capi.GeometricBAResult.from_buffer_copy(bufs["result"][1].tobytes())
    assert res.iterations == iters
    cost, nvalid = C.c_double(), C.c_int32()
    capi._chk(lib.dsopp_hip_geometric_ba_evaluate(h, C.byref(problem), C.c_double(1.5), C.byref(cost), C.byref(nvalid),
                                                  C.c_void_p(bufs["e_valid"][1].ctypes.data), C.c_void_p(bufs["e_res"][1].ctypes.data),
                                                  C.c_void_p(bufs["e_w"][1].ctypes.data)))
    capi._chk(lib.dsopp_hip_geometric_ba_flag_outliers(h, C.byref(problem), C.c_double(0.5), C.c_void_p(bufs["flags"][1].ctypes.data), None))
    has = np.zeros(L, np.uint8)
    capi._chk(lib.dsopp_hip_geometric_ba_triangulate(h, C.byref(problem), capi._p(has, np.uint8), 2, 0, C.c_void_p(bufs["triangulated"][1].ctypes.data)))
    for name, (whole, inner) in bufs.items():
        assert np.all(whole[:64] == 0xA5) and np.all(whole[64 + len(inner):] == 0xA5), name
        assert name == "triangulated" or not np.all(inner == 0xA5), name


def test_error_codes():
    pr = scene("F3_L63")[1]
    b = ba()

    def code(fn):
        with pytest.raises(capi.HipError) as e:
            fn()
        return int(str(e.value).split()[2].rstrip(":"))

    cam, poses, X, off, ofr, oxy = args(pr)
    # capacity: the 17th frame
    poses17 = np.tile(poses[:1], (17, 1))
    assert code(lambda: b.solve(cam, poses17, X, off, ofr, oxy)) == -5
    assert code(lambda: b.evaluate(cam, poses17, X, off, ofr, oxy)) == -5
    invalid = -1
    assert code(lambda: b.solve(cam, poses[:1], X, off, np.zeros_like(ofr), oxy)) == invalid            # one frame
    zero_t = poses.copy()
    zero_t[1, 9:] = 0.0
    assert code(lambda: b.solve(cam, zero_t, X, off, ofr, oxy)) == invalid                              # |t_1| = 0
    for bad in (np.nan, np.inf):
        for which in range(3):
            arrays = [poses.copy(), X.copy(), oxy.copy()]
            arrays[which][0, 0] = bad
            assert code(lambda: b.solve(cam, arrays[0], arrays[1], off, ofr, arrays[2])) == invalid
            assert code(lambda: b.evaluate(cam, arrays[0], arrays[1], off, ofr, arrays[2])) == invalid
            assert code(lambda: b.flag_outliers(cam, arrays[0], arrays[1], off, ofr, arrays[2])) == invalid
    assert code(lambda: b.solve((np.nan,) + tuple(cam[1:]), poses, X, off, ofr, oxy)) == invalid
    assert code(lambda: b.solve(cam[:4] + (8, 8), poses, X, off, ofr, oxy)) == invalid
    twice = ofr.copy()
    twice[1] = twice[0]
    assert code(lambda: b.solve(cam, poses, X, off, twice, oxy)) == invalid                             # a pair listed twice
    far = ofr.copy()
    far[0] = pr.F
    assert code(lambda: b.solve(cam, poses, X, off, far, oxy)) == invalid
    bad_off = off.copy()
    bad_off[1], bad_off[2] = off[2], off[1]
    assert code(lambda: b.evaluate(cam, poses, X, bad_off, ofr, oxy)) == invalid
    short = off.copy()
    short[-1] -= 1
    assert code(lambda: b.evaluate(cam, poses, X, short, ofr, oxy)) == invalid
    for field, value in (("a", 0.0), ("a", np.nan), ("lambda_0", -1.0), ("decrease_factor", 0.0), ("increase_factor", np.inf),
                         ("max_iterations", -1), ("iteration_group", -1), ("function_tolerance", np.nan)):
        assert code(lambda: b.solve(cam, poses, X, off, ofr, oxy, **{field: value})) == invalid, field
    assert code(lambda: b.evaluate(cam, poses, X, off, ofr, oxy, a=-1.0)) == invalid
    assert code(lambda: b.triangulate(cam, poses, X, off, ofr, oxy, np.zeros(pr.L, np.uint8), 1)) == invalid
    assert code(lambda: b.flag_outliers(cam, poses, X, off, ofr, oxy, np.nan)) == invalid
    lib = capi.lib()
    assert lib.dsopp_hip_geometric_ba_solve(None, None, None, None, None) == invalid
    assert lib.dsopp_hip_geometric_ba_solve(b._h, None, None, None, None) == invalid
    assert lib.dsopp_hip_geometric_ba_create(0, None, None) == invalid
    with pytest.raises(capi.HipError):
        capi.GeometricBA(device=1 << 20)
    # the object still works
    assert b.evaluate(cam, poses, X, off, ofr, oxy)["valid_residuals"] == gm.evaluate(pr)["nvalid"]


def test_no_iteration_and_no_observation():
    pr = scene("F3_L63")[1]
    ev = gm.evaluate(pr)
    out = ba().solve(*args(pr), debug=True, max_iterations=0)
    assert (out["iterations"], out["accepted_steps"], out["converged"], out["reason"]) == (0, 0, 0, 0)
    assert out["initial_cost"] == out["final_cost"] and abs(out["final_cost"] - ev["cost"]) <= 1e-10 * ev["cost"]
    assert out["valid_residuals"] == ev["nvalid"] and out["final_lambda"] == gm.LAMBDA_0 and out["trace"] == []
    assert np.array_equal(out["poses"], pr.poses) and np.array_equal(out["positions"], pr.X)
    assert np.array_equal(out["candidate_poses"], pr.poses) and not out["reduced_H"].any() and not out["pose_step"].any()
    assert np.array_equal(out["obs_valid"].astype(bool), ev["valid"])
    # M = 0: landmarks without observations, and no landmark at all
    for L in (3, 0):
        X = pr.X[:L]
        off, ofr, oxy = np.zeros(L + 1, np.int32), np.zeros(0, np.int32), np.zeros((0, 2))
        out = ba().solve(pr.cam, pr.poses, X, off, ofr, oxy, debug=True)
        assert (out["iterations"], out["reason"], out["final_cost"], out["valid_residuals"]) == (0, gm.NO_VALID_RESIDUAL, 0.0, 0)
        assert np.array_equal(out["poses"], pr.poses) and np.array_equal(out["positions"], X)
        ev0 = ba().evaluate(pr.cam, pr.poses, X, off, ofr, oxy, with_observations=True)
        assert (ev0["cost"], ev0["valid_residuals"]) == (0.0, 0)
        assert len(ba().flag_outliers(pr.cam, pr.poses, X, off, ofr, oxy)) == 0
        done, _ = ba().triangulate(pr.cam, pr.poses, X, off, ofr, oxy, np.zeros(L, np.uint8))
        assert not done.any()


def test_nothing_valid_ends_the_loop():
    """every point behind every camera: the driver's loop does not start"""
    pr = scene("F3_L63")[1]
    behind = pr.with_state(pr.poses, pr.X * [1.0, 1.0, -1.0])
    assert gm.evaluate(behind)["nvalid"] == 0
    out = ba().solve(*args(behind))
    model = gm.solve(behind)
    assert (out["iterations"], out["reason"], out["final_cost"]) == (0, gm.NO_VALID_RESIDUAL, 0.0) == (model["iterations"], model["reason"], model["final_cost"])


# ---- the host mirror and its driver

class DeviceBackend:
    """the three calls of a bootstrap frame on the device, for geometric_ba_model.run_bootstrap"""

    def triangulate(self, pr, has, min_projections, retriangulation):
        done, X = ba().triangulate(*args(pr), has, min_projections, retriangulation)
        return done.astype(bool), X

    def solve(self, pr, a):
        out = ba().solve(*args(pr), a=a)
        return out["poses"], out["positions"], dict(iterations=out["iterations"], accepted=out["accepted_steps"], reason=out["reason"],
                                                    valid=out["valid_residuals"], initial_cost=out["initial_cost"], final_cost=out["final_cost"])

    def flag_outliers(self, pr, threshold):
        return ba().flag_outliers(*args(pr), threshold)


@functools.lru_cache(maxsize=None)
def bootstrap_runs():
    track = gm.make_track()
    return track, gm.run_bootstrap(gm.ModelBackend(), track), gm.run_bootstrap(DeviceBackend(), track)


def track_distance(a, b):
    (af, al, _), (bf, bl, _) = a, b
    dp = max(np.abs(x["t_world_agent"] - y["t_world_agent"]).max() for x, y in zip(af, bf))
    dx = max(np.abs(x["X"] - y["X"]).max() for x, y in zip(al, bl) if x["has"])
    return max(dp, dx)


COUNTS = ("triangulated", "removed", "iterations", "accepted", "reason", "valid")


def test_three_bootstrap_frames_against_the_model():
    """triangulate, optimise, prune, three times, each step fed by the one before: the device's track stays with the model's.  The bar is
    the full solve's: d = the distance of the float64 and the longdouble model compositions, which agree on every count for this track."""
    track, model, device = bootstrap_runs()
    extended = gm.run_bootstrap(gm.ModelBackend(np.longdouble), track)
    (mf, ml, mrec), (df, dl, drec) = model, device
    counts = [[r[k] for k in COUNTS] for r in mrec]
    assert counts == [[r[k] for k in COUNTS] for r in extended[2]], "the track was chosen so that the model runs agree"
    assert all(r["iterations"] > 0 and r["removed"] > 0 for r in mrec) and sum(r["triangulated"] for r in mrec) > 0
    assert [[r[k] for k in COUNTS] for r in drec] == counts
    assert [lm["has"] for lm in dl] == [lm["has"] for lm in ml]
    assert [[fid for fid, _ in lm["proj"]] for lm in dl] == [[fid for fid, _ in lm["proj"]] for lm in ml]
    d, dist = track_distance(model, extended), track_distance(device, model)
    print(f"three bootstrap frames: d = {d:.3e}, device distance {dist:.3e}, bar {16 * max(d, 1e-12):.3e}")
    assert dist <= 16 * max(d, 1e-12)
    for a, b in zip(drec, mrec):
        assert abs(a["final_cost"] - b["final_cost"]) <= 1e-9 * b["final_cost"]


def test_driver_runs_the_host_mirror(tmp_path):
    """example_refine_track.cpp drives HipRefineTrack over the C-ABI alone: the same bytes as the Python binding composed the same way"""
    import subprocess
    import struct
    import test_geometric_ba as tgb
    track, _, (df, dl, drec) = bootstrap_runs()
    exe = tgb.build_example(tmp_path)
    path = str(tmp_path / "track.bin")
    gm.write_track_file(path, track, 3)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 15, r.stdout

    def doubles(words):
        return np.array([struct.unpack("<d", struct.pack("<Q", int(w, 16)))[0] for w in words])

    for step, rec in enumerate(drec):
        head, cost = lines[5 * step], lines[5 * step + 1].split()
        assert head == (f"step {step}: triangulated {rec['triangulated']}, iterations {rec['iterations']}, accepted {rec['accepted']}, "
                        f"reason {rec['reason']}, valid {rec['valid']}, removed {rec['removed']}"), head
        assert np.array_equal(doubles(cost[1:]), [rec["initial_cost"], rec["final_cost"]])
    poses = doubles(lines[12].split()[1:]).reshape(-1, 12)
    assert np.array_equal(poses, np.array([f["t_world_agent"] for f in df]))
    words = lines[13].split()[1:]
    for l, lm in enumerate(dl):
        assert int(words[4 * l]) == int(lm["has"])
        if lm["has"]:
            assert np.array_equal(doubles(words[4 * l + 1:4 * l + 4]), lm["X"]), l
    assert [int(w) for w in lines[14].split()[1:]] == [len(lm["proj"]) for lm in dl]
    # a file that ends early is an error, not a crash
    with open(path, "rb") as f:
        blob = f.read()
    with open(path, "wb") as f:
        f.write(blob[:len(blob) // 2])
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "too short" in r.stdout
