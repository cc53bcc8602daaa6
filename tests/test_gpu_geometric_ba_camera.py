"""The camera block of the device geometric bundle adjustment (dsopp_hip_geometric_ba_evaluate_camera / _solve_camera,
capi.GeometricBA.evaluate_camera / solve_camera) against its NumPy statement (tests/geometric_ba_camera_model.py), on the scenes of
tests/test_gpu_geometric_ba.py.  The bars are that file's, taken over:
  evaluate      validity equal (no decision lies within 1e-9 of a threshold but the hand-made ones: asserted on the model), residuals within
                1e-9 px, cost within 1e-10 relative
  pinning       a pinhole with every intrinsic fixed and free poses and landmarks: the bytes of dsopp_hip_geometric_ba_solve
  one iteration dr/dc within 1e-9 of its row's largest entry; the reduced system within 1e-9 sqrt(H_ii H_jj) of the undamped diagonal, camera
                rows included; the right-hand side within 1e-9 sqrt(H_ii sum w r^2); the step's backward error against the device's own
                system within dsm.working_threshold(omega_lapack); candidate poses, positions (to 1 + |X|), intrinsics (to 1 + |c|) and
                cost (to the cost before) at 1e-12 from the model applied to the device's own step.  Poses that are fixed are the scene's
                true ones (iteration_problem says why), and every case asserts that the float64 model is itself within half of 1e-12 of
                its longdouble run
                The scene's own start with FIX_POSES (wrong poses) is a test of its own, at 16 max(d, 1e-12) with d that distance
  full solve    all free and with fixed blocks (SOLVES): iteration count, accept pattern and reason equal; the final state, intrinsics relative to 1 + |c_i|, within
                16 max(d, 1e-12), d = the distance of the float64 and the longdouble model runs, which agree on the pattern (asserted);
                no case is left out
A simple-radial scene is the pinhole scene with every observation moved by the distortion of its true projection, noise and outliers kept."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_remap_model as crm
import dense_solve_model as dsm
import geometric_ba_camera_model as gc
import geometric_ba_model as gm
import test_gpu_geometric_ba as base
from dsopp_amd import capi

pytestmark = pytest.mark.gpu

ba = base.ba
K_TRUE = (-0.12, 0.03)
FIX_ALL_INTRINSICS = gc.FIX_FOCAL | gc.FIX_CENTER | gc.FIX_MODEL_SPECIFIC


def state(pr):
    return np.asarray(pr.poses, np.float64), np.asarray(pr.X, np.float64), pr.off, pr.ofr, pr.oxy


def size(pr):
    return pr.cam[4], pr.cam[5]


def base_scene(name):
    return base.one_observation_scene() if name == "one_observation" else base.scene(name)


@functools.lru_cache(maxsize=None)
def camera_scene(name, model):
    """(start Problem, true intrinsics, start intrinsics): the scene's perturbed state with a camera that is off the truth too"""
    truth, start = base_scene(name)
    fx, fy, cx, cy = truth.cam[:4]
    if model == gc.PINHOLE:
        return start, np.array([fx, fy, cx, cy]), np.array([fx * 1.01, fy * 0.99, cx + 2.0, cy - 1.5])
    true_c = np.array([fx, cx, cy, K_TRUE[0], K_TRUE[1]])
    _, q_pinhole, _ = gm.project(truth)
    valid, q_radial, _ = gc.project(truth, gc.Camera(gc.SIMPLE_RADIAL, true_c))
    assert valid.all()
    pr = gm.Problem(start.cam, start.poses, start.X, start.off, start.ofr, q_radial + (truth.oxy - q_pinhole))
    return pr, true_c, true_c + np.array([fx * 0.01, 2.0, -1.5, 0.02, -0.01])


def assert_no_near_decision(pr, cam):
    first, edge = gc.decision_margins(pr, cam)
    assert first.min() > 1e-9 and edge.min() > 1e-9, (first.min(), edge.min())


# ---- evaluate

@pytest.mark.parametrize("model", [gc.PINHOLE, gc.SIMPLE_RADIAL])
@pytest.mark.parametrize("name", ["F2_L40", "F3_L63", "F16_L65", "F10_L3000", "F5_L120_outliers", "one_observation"])
def test_evaluate(name, model):
    pr, _, c0 = camera_scene(name, model)
    cam = gc.Camera(model, c0)
    assert_no_near_decision(pr, cam)
    ev = gc.evaluate(pr, cam)
    out = ba().evaluate_camera(size(pr), model, c0, *state(pr), with_observations=True)
    assert np.array_equal(out["obs_valid"].astype(bool), ev["valid"]) and out["valid_residuals"] == ev["nvalid"] > 0
    err = np.abs(out["obs_residual"] - ev["r"]).max()
    rel = abs(out["cost"] - ev["cost"]) / ev["cost"]
    radius = gc.max_valid_radius(pr, cam)
    print(f"{name} model {model}: residual error {err:.3e} px, cost relative error {rel:.3e}, radius {out['max_valid_radius']!r} / {radius!r}")
    assert err <= 1e-9 and rel <= 1e-10
    assert np.abs(out["obs_weight"] - ev["w"]).max() <= 1e-12
    assert abs(out["max_valid_radius"] - radius) <= 1e-12 * radius


def radial_edge_problem():
    """Frame 0 is the identity and the camera's constants are exact, so that u = X_x of the hand-made points; the camera's radius comes
    from the extremum rule (a square root, a division, a difference: the same bytes in the model and in the library), so the decision AT
    the radius is compared, not left out.  One observation each, in frame 0.  Landmark 0: sqrt(rho2) exactly the radius (valid);
    1: one ulp beyond (invalid); 2: behind the camera, and valid all the same: the simple-radial projection has no test on p_z;
    3: p_z = 0, q is not finite (invalid); 4: an ordinary point."""
    cam = gc.Camera(gc.SIMPLE_RADIAL, [128.0, 128.0, 128.0, -0.6, 0.05])
    shape = (0.0, 0.0, 0.0, 0.0, 256, 256)
    derived, replaced = crm.simple_radial_derived(256, 256, *cam.c)
    assert replaced
    radius = float(derived[0])
    poses = np.zeros((2, 12))
    poses[:, [0, 4, 8]] = 1.0
    poses[1, 9:] = [0.25, 0.0, 0.5]
    X = np.array([[radius, 0.0, 1.0], [np.nextafter(radius, 2.0), 0.0, 1.0], [-0.1, -0.05, -1.0], [0.1, 0.1, 0.0], [0.2, 0.1, 2.0]])
    pr = gm.Problem(shape, poses, X, np.arange(6), np.zeros(5, np.int32), np.zeros((5, 2)))
    _, q, _ = gc.project(pr, cam)
    return gm.Problem(shape, poses, X, np.arange(6), np.zeros(5, np.int32), np.where(np.isfinite(q), q + 0.25, 0.0)), cam, radius


def test_evaluate_simple_radial_at_the_thresholds():
    pr, cam, radius = radial_edge_problem()
    ev = gc.evaluate(pr, cam)
    assert ev["valid"].tolist() == [True, False, True, False, True]          # the model decides as designed
    out = ba().evaluate_camera(size(pr), cam.model, cam.c, *state(pr), with_observations=True)
    assert out["max_valid_radius"] == radius
    assert np.array_equal(out["obs_valid"].astype(bool), ev["valid"])
    assert np.abs(out["obs_residual"] - ev["r"]).max() <= 1e-9
    assert np.all(out["obs_residual"][~ev["valid"]] == 0.0) and np.all(out["obs_weight"][~ev["valid"]] == 0.0)
    assert abs(out["cost"] - ev["cost"]) <= 1e-10 * ev["cost"]


# ---- the pinning property

@pytest.mark.parametrize("name", ["F3_L63", "F16_L65", "F5_L120_outliers"])
def test_all_intrinsics_fixed_is_the_solver_without_a_camera_block(name):
    pr = base.scene(name)[1]
    old = ba().solve(*base.args(pr), debug=True)
    new = ba().solve_camera(size(pr), gc.PINHOLE, pr.cam[:4], *state(pr), fixed=FIX_ALL_INTRINSICS, debug=True)
    assert old["iterations"] > 1
    for key in ("poses", "positions", "reduced_H", "reduced_b", "pose_step", "candidate_poses", "candidate_positions", "landmark_H", "obs_residual"):
        assert old[key].tobytes() == new[key].tobytes(), key
    result = [name for name, _ in capi.GeometricBAResult._fields_ if name != "reserved"]
    assert [old[k] for k in result] == [new[k] for k in result]
    assert np.array(old["trace"]).tobytes() == np.array(new["trace"]).tobytes()
    assert np.array_equal(new["intrinsics"], pr.cam[:4]) and new["max_valid_radius"] == 0.0


# ---- one iteration

CONFIGS = {"pinhole_focal": (gc.PINHOLE, gc.FIX_CENTER), "pinhole_centre": (gc.PINHOLE, gc.FIX_FOCAL), "pinhole_all": (gc.PINHOLE, 0),
           "radial_all": (gc.SIMPLE_RADIAL, 0), "radial_model_specific": (gc.SIMPLE_RADIAL, gc.FIX_FOCAL | gc.FIX_CENTER),
           "fixed_landmarks": (gc.SIMPLE_RADIAL, gc.FIX_LANDMARKS | FIX_ALL_INTRINSICS), "fixed_poses": (gc.SIMPLE_RADIAL, gc.FIX_POSES),
           "camera_only": (gc.PINHOLE, gc.FIX_POSES | gc.FIX_LANDMARKS),
           # fixed landmarks with free poses AND a free camera: H_pc enters the system without a Schur part
           "fixed_landmarks_free_camera": (gc.SIMPLE_RADIAL, gc.FIX_LANDMARKS),
           # landmarks only: no reduced system at all (n = 0), every landmark steps by -(H_ll + lambda D)^-1 b_l
           "landmarks_only": (gc.SIMPLE_RADIAL, gc.FIX_POSES | FIX_ALL_INTRINSICS)}
ITERATION_SCENES = ["F2_L40", "F3_L63", "F10_L64", "F16_L65", "F5_L300", "F10_L3000", "one_observation"]


def iteration_problem(name, model, fixed, wrong_poses=False):
    """the scene's start; poses that are fixed are poses that are known: with FIX_POSES they are the scene's true ones.  (Landmarks that
    make up for fixed WRONG poses take steps of several units along rays that a single observation does not constrain; the float64 model
    then lies up to 4e-12 from its own longdouble run, and no float64 code can be held to 1e-12 of it.  test_one_iteration asserts for
    every case that the model is within half of the bar of its longdouble self;
    test_one_iteration_with_fixed_wrong_poses keeps the scene's own start, with the bar that distance gives.)"""
    pr, _, c0 = camera_scene(name, model)
    if fixed & gc.FIX_POSES and not wrong_poses:
        pr = pr.with_state(base_scene(name)[0].poses, pr.X)
    return pr, c0


@functools.lru_cache(maxsize=8)
def linearisation(name, model, true_poses, dtype=np.float64):
    pr, c0 = iteration_problem(name, model, gc.FIX_POSES if true_poses else 0)
    return gc.linearise(pr, gc.Camera(model, c0), dtype=dtype)


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("name", ITERATION_SCENES)
def test_one_iteration(name, config):
    from scipy.linalg import cho_factor, cho_solve
    model, fixed = CONFIGS[config]
    pr, c0 = iteration_problem(name, model, fixed)
    cam = gc.Camera(model, c0, fixed)
    assert_no_near_decision(pr, cam)
    npose, free, moves = gc.unknowns(model, fixed, pr.F)
    n = npose + len(free)
    lam = gm.LAMBDA_0
    norm1 = np.linalg.norm(pr.poses[1, 9:])
    lin = linearisation(name, model, bool(fixed & gc.FIX_POSES))
    H, g, extra = gc.reduced_system(pr, cam, lin, lam, norm1)
    out = ba().solve_camera(size(pr), model, c0, *state(pr), fixed=fixed, debug=True, max_iterations=1)
    assert out["iterations"] == 1 and out["system_lambda"] == lam and out["reduced_H"].shape == (n, n) == H.shape
    # the linearisation
    assert np.array_equal(out["obs_valid"].astype(bool), lin["valid"])
    eJ = np.abs(out["obs_camera_jacobian"] - lin["Jc"])
    row = np.abs(lin["Jc"]).max(-1, keepdims=True)
    assert np.all(eJ <= 1e-9 * row), (eJ / np.maximum(row, 1e-300)).max()
    assert np.all(out["obs_camera_jacobian"][~lin["valid"]] == 0.0)
    wr2 = float(np.sum(lin["w"] * np.sum(lin["r"] ** 2, -1)))
    dp = np.sqrt(extra["diag"])
    eS, eg = np.abs(out["reduced_H"] - H), np.abs(out["reduced_b"] - g)
    x = out["pose_step"]
    assert np.all(np.isfinite(x)) and gm.cholesky_solve(H, g) is not None
    if n:                                            # (landmarks only: there is no system and no step to judge)
        print(f"{name} {config}: n = {n}, reduced system error {(eS / np.outer(dp, dp)).max():.3e}, right-hand side {(eg / (dp * np.sqrt(wr2))).max():.3e}")
        assert np.all(eS <= 1e-9 * np.outer(dp, dp))
        assert np.all(eg <= 1e-9 * dp * np.sqrt(wr2))
        # the step: backward error against the device's own system
        omega = base.backward_error(out["reduced_H"], out["reduced_b"], x)
        omega_lapack = base.backward_error(out["reduced_H"], out["reduced_b"], cho_solve(cho_factor(out["reduced_H"], lower=True), out["reduced_b"]))
        print(f"{name} {config}: omega {omega:.3e}, omega_lapack {omega_lapack:.3e}")
        assert omega <= dsm.working_threshold(omega_lapack), (omega, omega_lapack)
    # the rest of the iteration, from the device's own step
    st = gc.apply_step(pr, cam, lin, lam, norm1, x)
    assert st["camera_ok"]
    cand = st["candidate"]
    # the case can be judged at 1e-12: the float64 model applied to this step lies within half of that of its longdouble run, which leaves
    # the other half to a device that rounds as often as the model does
    ext = gc.apply_step(pr, cam, linearisation(name, model, bool(fixed & gc.FIX_POSES), np.longdouble), lam, norm1, x, dtype=np.longdouble)
    own = max(float(np.abs(cand.poses - ext["candidate"].poses).max()), float((np.abs(cand.X - ext["candidate"].X) / (1.0 + np.abs(cand.X))).max()),
              float(abs(st["cost"] - ext["cost"]) / lin["cost"]))
    assert own <= 0.5e-12, own
    ep = np.abs(out["candidate_poses"] - cand.poses).max()
    ex = (np.abs(out["candidate_positions"] - cand.X) / (1.0 + np.abs(cand.X))).max()
    full = np.zeros(5)
    full[:len(c0)] = st["camera"].c
    ei = (np.abs(out["candidate_intrinsics"] - full) / (1.0 + np.abs(full))).max()
    cost_before, cost_candidate, accepted, lam_used = out["trace"][0]
    ec = abs(cost_candidate - st["cost"]) / cost_before
    print(f"{name} {config}: candidate poses {ep:.3e}, positions {ex:.3e}, intrinsics {ei:.3e} relative, cost {ec:.3e} of the cost before")
    assert ep <= 1e-12 and ex <= 1e-12 and ei <= 1e-12 and ec <= 1e-12
    assert lam_used == lam and abs(cost_before - lin["cost"]) <= 1e-10 * lin["cost"]
    if not npose:
        assert np.array_equal(out["candidate_poses"], pr.poses)
    if not moves:
        assert np.array_equal(out["candidate_positions"], pr.X)
    fixed_slots = [k for k in range(len(c0)) if k not in free]
    assert np.array_equal(out["candidate_intrinsics"][fixed_slots], c0[fixed_slots])
    if model == gc.SIMPLE_RADIAL:
        radius = gc.max_valid_radius(pr, st["camera"])
        assert abs(out["candidate_max_valid_radius"] - radius) <= 1e-12 * radius
    # what the call hands back is the accepted candidate, or the state
    kept = out["candidate_intrinsics"][:len(c0)] if accepted else c0
    assert np.array_equal(out["intrinsics"], kept)


@pytest.mark.parametrize("name", ITERATION_SCENES)
def test_one_iteration_with_fixed_wrong_poses(name):
    """FIX_POSES on the scene's own perturbed start: the landmarks make up for poses that are wrong, and those seen once step several units
    along their rays, a direction only the damping holds.  The float64 model applied to the device's step lies up to 4e-12 from its own
    longdouble run there (F10_L3000 4e-13, one_observation 4e-12), so the candidate is held to the full solve's derived bar,
    16 max(d, 1e-12) with d that distance, not to 1e-12.  (Measured on the device before this bar stood: 1.4e-12 and 1.7e-11.)"""
    model, fixed = CONFIGS["fixed_poses"]
    pr, c0 = iteration_problem(name, model, fixed, wrong_poses=True)
    cam = gc.Camera(model, c0, fixed)
    assert_no_near_decision(pr, cam)
    lam = gm.LAMBDA_0
    lin = gc.linearise(pr, cam)
    out = ba().solve_camera(size(pr), model, c0, *state(pr), fixed=fixed, debug=True, max_iterations=1)
    x = out["pose_step"]
    st = gc.apply_step(pr, cam, lin, lam, None, x)
    ext = gc.apply_step(pr, cam, gc.linearise(pr, cam, dtype=np.longdouble), lam, None, x, dtype=np.longdouble)
    cand = st["candidate"]
    d = max(float((np.abs(cand.X - ext["candidate"].X) / (1.0 + np.abs(cand.X))).max()), float(abs(st["cost"] - ext["cost"]) / lin["cost"]))
    ex = (np.abs(out["candidate_positions"] - cand.X) / (1.0 + np.abs(cand.X))).max()
    ec = abs(out["trace"][0][1] - st["cost"]) / out["trace"][0][0]
    print(f"{name}: d = {d:.3e}, candidate positions {ex:.3e} relative, cost {ec:.3e} of the cost before, bar {16 * max(d, 1e-12):.3e}")
    assert max(ex, ec) <= 16 * max(d, 1e-12)
    assert np.array_equal(out["candidate_poses"], pr.poses)
    assert (np.abs(out["candidate_intrinsics"] - st["camera"].c) / (1.0 + np.abs(st["camera"].c))).max() <= 1e-12


# ---- the full solve

# all free, and runs in which something is fixed, to their end: (scene, model, fixed).  FIX_LANDMARKS with every intrinsic fixed is the run
# whose end hangs on the state norm: fixed landmarks have no part in it, and with sum |X|^2 counted the parameter tolerance would be met
# 4 to 6 iterations early on these scenes
SOLVES = [(name, model, 0) for name in ("F3_L63", "F10_L64", "F16_L65", "F5_L120_outliers") for model in (gc.PINHOLE, gc.SIMPLE_RADIAL)] + \
         [(name, gc.SIMPLE_RADIAL, gc.FIX_LANDMARKS | FIX_ALL_INTRINSICS) for name in ("F3_L63", "F10_L64", "F5_L120_outliers")] + \
         [("F3_L63", gc.SIMPLE_RADIAL, gc.FIX_LANDMARKS), ("F10_L64", gc.PINHOLE, gc.FIX_LANDMARKS),
          ("F3_L63", gc.PINHOLE, gc.FIX_POSES | gc.FIX_LANDMARKS), ("F5_L120_outliers", gc.SIMPLE_RADIAL, gc.FIX_POSES | gc.FIX_LANDMARKS),
          ("F3_L63", gc.SIMPLE_RADIAL, gc.FIX_POSES | FIX_ALL_INTRINSICS), ("F10_L64", gc.SIMPLE_RADIAL, gc.FIX_POSES | FIX_ALL_INTRINSICS)]


@functools.lru_cache(maxsize=None)
def model_pair(name, model, fixed):
    pr, _, c0 = camera_scene(name, model)
    a = gc.solve(pr, gc.Camera(model, c0, fixed))
    b = gc.solve(pr, gc.Camera(model, c0, fixed), dtype=np.longdouble)
    pattern = [t[2] for t in a["trace"]]
    assert a["iterations"] == b["iterations"] and pattern == [t[2] for t in b["trace"]], "the start was chosen so that the model runs agree"
    d = max(float(np.abs(a["problem"].poses - b["problem"].poses).max()), float(np.abs(a["problem"].X - b["problem"].X).max()),
            float((np.abs(a["camera"].c - b["camera"].c) / (1.0 + np.abs(a["camera"].c))).max()))
    return a, pattern, d


@pytest.mark.parametrize("name,model,fixed", SOLVES)
def test_full_solve(name, model, fixed):
    a, pattern, d = model_pair(name, model, fixed)
    pr, _, c0 = camera_scene(name, model)
    out = ba().solve_camera(size(pr), model, c0, *state(pr), fixed=fixed, debug=True)
    ca = np.asarray(a["camera"].c, np.float64)
    dist = max(np.abs(out["poses"] - a["problem"].poses).max(), np.abs(out["positions"] - a["problem"].X).max(),
               (np.abs(out["intrinsics"] - ca) / (1.0 + np.abs(ca))).max())
    print(f"{name} model {model} fixed {fixed}: {out['iterations']} iterations, reason {out['reason']}, d = {d:.3e}, device distance {dist:.3e}, bar {16 * max(d, 1e-12):.3e}, "
          f"intrinsics {out['intrinsics']}")
    assert out["iterations"] == a["iterations"] and [t[2] for t in out["trace"]] == pattern
    assert out["reason"] == a["reason"] and out["converged"] == int(a["converged"]) and out["accepted_steps"] == a["accepted"]
    assert dist <= 16 * max(d, 1e-12)
    assert abs(out["final_cost"] - a["final_cost"]) <= 1e-9 * a["final_cost"] and out["valid_residuals"] == a["nvalid"]
    assert out["final_lambda"] == float(a["lambda"])
    if model == gc.SIMPLE_RADIAL:
        radius = gc.max_valid_radius(pr, a["camera"])
        assert abs(out["max_valid_radius"] - radius) <= 1e-9 * radius


# ---- a rejected candidate camera

def test_a_candidate_camera_without_a_focal_length_is_rejected():
    """Every landmark mirrored through the optical axis, poses, landmarks, centre and distortion fixed: the observations then correlate
    negatively with the rays, and the least-squares focal length is about -f.  The system is the focal length's own diagonal, so nothing
    here is near a decision: the model's first four candidates have f <= 0 and are rejected with an infinite cost, the damping grows tenfold
    each time until a candidate keeps f > 0, and the device goes the same way."""
    pr, true_c, _ = camera_scene("F3_L63", gc.SIMPLE_RADIAL)
    pr = pr.with_state(pr.poses, pr.X * [-1.0, -1.0, 1.0])
    cam = gc.Camera(gc.SIMPLE_RADIAL, true_c, gc.FIX_POSES | gc.FIX_LANDMARKS | gc.FIX_CENTER | gc.FIX_MODEL_SPECIFIC)
    assert_no_near_decision(pr, cam)
    lin = gc.linearise(pr, cam)
    H, g, _ = gc.reduced_system(pr, cam, lin, gm.LAMBDA_0, None)
    first = gc.apply_step(pr, cam, lin, gm.LAMBDA_0, None, gm.cholesky_solve(H, g))
    assert first["camera"].c[0] < -100.0 and not first["camera_ok"]
    run = gc.solve(pr, cam, max_iterations=8)
    pattern = [(bool(np.isinf(t[1])), t[2]) for t in run["trace"]]
    assert pattern[:5] == [(True, 0)] * 4 + [(False, 1)], pattern
    out = ba().solve_camera(size(pr), cam.model, true_c, *state(pr), fixed=cam.fixed, debug=True, max_iterations=8)
    print(f"rejected candidates: model {pattern}, f {run['camera'].c[0]!r}; device f {out['intrinsics'][0]!r}")
    assert [(bool(np.isinf(t[1])), t[2]) for t in out["trace"]] == pattern and out["iterations"] == run["iterations"] == 8
    assert out["trace"][0][0] == out["initial_cost"] and [t[3] for t in out["trace"]] == [float(t[3]) for t in run["trace"]]
    assert np.all(np.isfinite(out["intrinsics"])) and out["intrinsics"][0] > 0.0 and np.isfinite(out["final_cost"]) and out["max_valid_radius"] > 0.0
    assert abs(out["intrinsics"][0] - run["camera"].c[0]) <= 1e-9 * run["camera"].c[0]
    assert np.array_equal(out["intrinsics"][1:], true_c[1:]) and np.array_equal(out["poses"], pr.poses) and np.array_equal(out["positions"], pr.X)
    # one iteration alone: the state comes back untouched, the failing candidate is handed out as computed
    one = ba().solve_camera(size(pr), cam.model, true_c, *state(pr), fixed=cam.fixed, debug=True, max_iterations=1)
    assert np.array_equal(one["intrinsics"], true_c) and one["accepted_steps"] == 0 and one["final_lambda"] == gm.LAMBDA_0 * gm.INCREASE
    assert abs(one["candidate_intrinsics"][0] - first["camera"].c[0]) <= 1e-9 * abs(first["camera"].c[0])


# ---- housekeeping

def code(fn):
    with pytest.raises(capi.HipError) as e:
        fn()
    return int(str(e.value).split()[2].rstrip(":"))


def test_error_codes():
    pr, _, c0 = camera_scene("F3_L63", gc.SIMPLE_RADIAL)
    b, sz, st = ba(), size(pr), state(pr)
    invalid = -1
    for call in (b.evaluate_camera, b.solve_camera):
        assert code(lambda: call(sz, 2, c0, *st)) == invalid                                    # an unknown model
        assert code(lambda: call(sz, gc.SIMPLE_RADIAL, c0, *st, fixed=32)) == invalid           # an unknown bit
        for bad in (np.nan, np.inf):
            for k in range(5):
                c = c0.copy()
                c[k] = bad
                assert code(lambda: call(sz, gc.SIMPLE_RADIAL, c, *st)) == invalid
        for model, k in ((gc.SIMPLE_RADIAL, 0), (gc.PINHOLE, 0), (gc.PINHOLE, 1)):
            for focal in (0.0, -300.0):
                c = (c0 if model == gc.SIMPLE_RADIAL else np.array(pr.cam[:4])).copy()
                c[k] = focal
                assert code(lambda: call(sz, model, c, *st)) == invalid
        # a camera whose max_valid_radius is not finite: r - 40 r^3 never reaches the image corner and k2 = 0 leaves the extremum rule idle
        c = np.array([2.0, 320.0, 240.0, -40.0, 0.0])
        with np.errstate(all="ignore"):
            assert not np.isfinite(gc.max_valid_radius(pr, gc.Camera(gc.SIMPLE_RADIAL, c)))
        assert code(lambda: call(sz, gc.SIMPLE_RADIAL, c, *st)) == invalid
        # and one whose max_valid_radius is negative: the first extremum of r - 40 r^3 + r^5 lies at 0.09, within 4 / f = 2 of the axis
        c = np.array([2.0, 320.0, 240.0, -40.0, 1.0])
        assert gc.max_valid_radius(pr, gc.Camera(gc.SIMPLE_RADIAL, c)) < 0.0
        assert code(lambda: call(sz, gc.SIMPLE_RADIAL, c, *st)) == invalid
        poses17 = np.tile(st[0][:1], (17, 1))
        assert code(lambda: call(sz, gc.SIMPLE_RADIAL, c0, poses17, *st[1:])) == -5             # capacity: the 17th frame
    # nothing free: solve alone
    everything = gc.FIX_POSES | gc.FIX_LANDMARKS | FIX_ALL_INTRINSICS
    assert code(lambda: b.solve_camera(sz, gc.SIMPLE_RADIAL, c0, *st, fixed=everything)) == invalid
    assert b.evaluate_camera(sz, gc.SIMPLE_RADIAL, c0, *st, fixed=everything)["valid_residuals"] > 0
    # a pinhole has no model-specific intrinsic: the bit frees nothing
    assert code(lambda: b.solve_camera(sz, gc.PINHOLE, pr.cam[:4], *st, fixed=gc.FIX_POSES | gc.FIX_LANDMARKS | gc.FIX_FOCAL | gc.FIX_CENTER)) == invalid
    # |t_1| = 0 is invalid only when the poses are free
    zero_t = st[0].copy()
    zero_t[1, 9:] = 0.0
    assert code(lambda: b.solve_camera(sz, gc.SIMPLE_RADIAL, c0, zero_t, *st[1:])) == invalid
    assert b.solve_camera(sz, gc.SIMPLE_RADIAL, c0, zero_t, *st[1:], fixed=gc.FIX_POSES, max_iterations=2)["iterations"] == 2
    # problem->fx .. cy are ignored
    lib = capi.lib()
    assert lib.dsopp_hip_geometric_ba_solve_camera(b._h, None, None, None, None, None) == invalid
    problem, keep = capi.GeometricBA.problem((np.nan, 0.0, np.inf, -1.0) + sz, *st)
    opt, res = capi.default_geometric_ba_options(max_iterations=1), capi.GeometricBAResult()
    assert lib.dsopp_hip_geometric_ba_solve_camera(b._h, C.byref(problem), None, C.byref(opt), C.byref(res), None) == invalid
    cam = capi.GeometricBA.camera_record(gc.SIMPLE_RADIAL, c0, 0)
    assert lib.dsopp_hip_geometric_ba_solve_camera(b._h, C.byref(problem), C.byref(cam), C.byref(opt), C.byref(res), None) == 0
    assert res.iterations == 1


def test_iteration_group_and_repeated_calls_return_identical_bytes():
    pr, _, c0 = camera_scene("F5_L120_outliers", gc.SIMPLE_RADIAL)
    keys = ("poses", "positions", "intrinsics", "reduced_H", "reduced_b", "pose_step", "obs_camera_jacobian", "candidate_intrinsics")

    def blob(out):
        return b"".join(out[k].tobytes() for k in keys) + repr((out["trace"], out["iterations"], out["final_cost"], out["max_valid_radius"])).encode()

    first = blob(ba().solve_camera(size(pr), gc.SIMPLE_RADIAL, c0, *state(pr), debug=True, iteration_group=1))
    other = capi.GeometricBA()
    for obj, group in ((ba(), 3), (other, 64), (ba(), 0), (other, 1)):
        assert blob(obj.solve_camera(size(pr), gc.SIMPLE_RADIAL, c0, *state(pr), debug=True, iteration_group=group)) == first, group
    other.close()


def test_guard_bytes_around_the_camera_outputs():
    pr, _, c0 = camera_scene("F3_L63", gc.SIMPLE_RADIAL)
    problem, keep = capi.GeometricBA.problem((0.0, 0.0, 0.0, 0.0) + size(pr), *state(pr))
    F, L, M = pr.F, pr.L, pr.M
    n = 6 * (F - 1) - 1 + 5
    iters = 3
    sizes = dict(obs_valid=M, obs_residual=16 * M, obs_weight=8 * M, landmark_H=48 * L, landmark_b=24 * L, reduced_H=8 * n * n, reduced_b=8 * n,
                 pose_step=8 * n, system_lambda=8, candidate_poses=96 * F, candidate_positions=24 * L,
                 trace=iters * C.sizeof(capi.GeometricBATrace), obs_camera_jacobian=80 * M, candidate_intrinsics=40,
                 candidate_max_valid_radius=8)
    bufs = {k: base.guarded(v) for k, v in sizes.items()}
    bufs.update(poses=base.guarded(96 * F), positions=base.guarded(24 * L), result=base.guarded(C.sizeof(capi.GeometricBAResult)),
                camera=base.guarded(C.sizeof(capi.GeometricBACamera)), e_camera=base.guarded(C.sizeof(capi.GeometricBACamera)),
                e_valid=base.guarded(M), e_res=base.guarded(16 * M), e_w=base.guarded(8 * M))
    bufs["poses"][1][:] = keep[0].view(np.uint8).reshape(-1)
    bufs["positions"][1][:] = keep[1].view(np.uint8).reshape(-1)
    record = bytes(capi.GeometricBA.camera_record(gc.SIMPLE_RADIAL, c0, 0))
    for key in ("camera", "e_camera"):
        bufs[key][1][:] = np.frombuffer(record, np.uint8)
    problem.poses, problem.positions = bufs["poses"][1].ctypes.data, bufs["positions"][1].ctypes.data
    dbg = capi.GeometricBACameraDebug(capi.GeometricBADebug(*[bufs[name][1].ctypes.data for name in capi.GEOMETRIC_BA_DEBUG_FIELDS]),
                                      *[bufs[name][1].ctypes.data for name in capi.GEOMETRIC_BA_CAMERA_DEBUG_FIELDS])
    opt = capi.default_geometric_ba_options(max_iterations=iters)
    h, lib = ba()._h, capi.lib()
    capi._chk(lib.dsopp_hip_geometric_ba_solve_camera(h, C.byref(problem), C.c_void_p(bufs["camera"][1].ctypes.data), C.byref(opt),
                                                      C.c_void_p(bufs["result"][1].ctypes.data), C.byref(dbg)))
    assert capi.GeometricBAResult.from_buffer_copy(bufs["result"][1].tobytes()).iterations == iters
    cost, nvalid = C.c_double(), C.c_int32()
    capi._chk(lib.dsopp_hip_geometric_ba_evaluate_camera(h, C.byref(problem), C.c_void_p(bufs["e_camera"][1].ctypes.data), C.c_double(1.5),
                                                         C.byref(cost), C.byref(nvalid), C.c_void_p(bufs["e_valid"][1].ctypes.data),
                                                         C.c_void_p(bufs["e_res"][1].ctypes.data), C.c_void_p(bufs["e_w"][1].ctypes.data)))
    for name, (whole, inner) in bufs.items():
        assert np.all(whole[:64] == 0xA5) and np.all(whole[64 + len(inner):] == 0xA5), name
        assert not np.all(inner == 0xA5), name
    after = capi.GeometricBACamera.from_buffer_copy(bufs["camera"][1].tobytes())
    assert after.max_valid_radius > 0.0 and list(after.intrinsics) != list(c0)


# ---- the host mirror and its driver

class CameraBackend(base.DeviceBackend):
    """a bootstrap frame's three calls with the refinement in its OPTIMIZE_CAMERA form, as example_refine_track's switches compose them:
    triangulation with the intrinsics so far, solve_camera, pruning with the intrinsics it left"""

    def __init__(self, model, intrinsics, fixed):
        self.model, self.c, self.fixed, self.history = model, np.array(intrinsics, np.float64), fixed, []

    def with_camera(self, pr):
        """triangulation and pruning are the pinhole's: (f, f, cx, cy) of a simple-radial camera"""
        out = pr.with_state(pr.poses, pr.X)
        out.cam = (tuple(self.c) if self.model == gc.PINHOLE else (self.c[0], self.c[0], self.c[1], self.c[2])) + tuple(pr.cam[4:])
        return out

    def triangulate(self, pr, has, min_projections, retriangulation):
        return super().triangulate(self.with_camera(pr), has, min_projections, retriangulation)

    def solve(self, pr, a):
        out = ba().solve_camera(size(pr), self.model, self.c, *state(pr), fixed=self.fixed, a=a)
        self.history.append((self.c.copy(), out["intrinsics"].copy()))
        self.c = out["intrinsics"].copy()
        return out["poses"], out["positions"], dict(iterations=out["iterations"], accepted=out["accepted_steps"], reason=out["reason"],
                                                    valid=out["valid_residuals"], initial_cost=out["initial_cost"], final_cost=out["final_cost"])

    def flag_outliers(self, pr, threshold):
        return super().flag_outliers(self.with_camera(pr), threshold)


@pytest.mark.parametrize("model,switches,fixed", [(gc.PINHOLE, ["--free-focal", "--free-center"], gc.FIX_MODEL_SPECIFIC),
                                                  (gc.SIMPLE_RADIAL, ["--simple-radial", "--free-focal", "--free-distortion"], gc.FIX_CENTER)])
def test_driver_frees_the_intrinsics_through_the_host_mirror(tmp_path, model, switches, fixed):
    """example_refine_track with its camera switches drives HipRefineTrack's OPTIMIZE_CAMERA overload, for either camera model, over the
    C-ABI alone: the same bytes as solve_camera composed the same way through the Python binding"""
    import struct
    import subprocess
    import test_geometric_ba as tgb
    track = gm.make_track()
    fx, fy, cx, cy = track[0][:4]
    count = 4 if model == gc.PINHOLE else 5
    backend = CameraBackend(model, [fx, fy, cx, cy] if model == gc.PINHOLE else [fx, cx, cy, 0.0, 0.0], fixed)
    frames, landmarks, records = gm.run_bootstrap(backend, track)
    free = gc.free_intrinsics(model, fixed)
    assert len(backend.history) == 3 and all(np.all(before[free] != after[free]) for before, after in backend.history)
    exe = tgb.build_example(tmp_path)
    path = str(tmp_path / "track.bin")
    gm.write_track_file(path, track, 3)
    r = subprocess.run([exe, path] + switches, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 21, r.stdout

    def doubles(words):
        return np.array([struct.unpack("<d", struct.pack("<Q", int(w, 16)))[0] for w in words])

    for step, (rec, (before, after)) in enumerate(zip(records, backend.history)):
        block = lines[7 * step:7 * step + 7]
        assert block[0].startswith("intrinsics before ") and np.array_equal(doubles(block[0].split()[2:2 + count]), before)
        assert block[1].startswith("intrinsics after ") and np.array_equal(doubles(block[1].split()[2:2 + count]), after)
        assert block[2] == (f"step {step}: triangulated {rec['triangulated']}, iterations {rec['iterations']}, accepted {rec['accepted']}, "
                            f"reason {rec['reason']}, valid {rec['valid']}, removed {rec['removed']}"), block[2]
        assert np.array_equal(doubles(block[3].split()[1:]), [rec["initial_cost"], rec["final_cost"]])
    assert np.array_equal(doubles(lines[18].split()[1:]).reshape(-1, 12), np.array([f["t_world_agent"] for f in frames]))
    words = lines[19].split()[1:]
    for l, lm in enumerate(landmarks):
        assert int(words[4 * l]) == int(lm["has"])
        if lm["has"]:
            assert np.array_equal(doubles(words[4 * l + 1:4 * l + 4]), lm["X"]), l
    assert [int(w) for w in lines[20].split()[1:]] == [len(lm["proj"]) for lm in landmarks]
    # without a switch the driver prints what it printed before; an unknown switch, or distortion freed on a pinhole, is the usage line
    plain = subprocess.run([exe, path], capture_output=True, text=True, timeout=60)
    assert plain.returncode == 0 and len(plain.stdout.strip().split("\n")) == 15 and "intrinsics" not in plain.stdout
    assert subprocess.run([exe, path, "--free-everything"], capture_output=True, text=True, timeout=60).returncode == 1
    assert subprocess.run([exe, path, "--free-distortion"], capture_output=True, text=True, timeout=60).returncode == 1
