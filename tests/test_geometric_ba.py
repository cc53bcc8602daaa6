"""tests/geometric_ba_model.py, the NumPy statement of the bootstrap's geometric bundle adjustment (include/dsopp_hip.h,
dsopp_hip_geometric_ba_*), pinned on the CPU: the Jacobians against central differences, the Schur step against a dense solve of the whole
damped normal equations, the ground truth of a noise-free scene, the stationarity of the robust cost among gross outliers, exact
triangulation, the pruning rule, and the track composition of the host mirror.  tests/test_gpu_geometric_ba.py holds the device to it."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geometric_ba_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def retract(pr, norm1, x):
    """the state moved by the reduced pose step x and no landmark step: the chart the Jacobians are taken in"""
    lin = {"Hll": np.zeros((pr.L, 3, 3)), "bl": np.zeros((pr.L, 3)), "C": np.zeros((pr.M, 3, 3))}
    return gm.apply_step(pr, lin, 0.0, norm1, x)["candidate"]


def residual_vector(pr):
    return gm.evaluate(pr)["r"].reshape(-1)


def test_jacobians_against_central_differences():
    truth, rng = gm.make_scene(F=4, L=12, seed=1, noise=0.5)
    pr = gm.perturb(truth, rng)
    norm1 = np.linalg.norm(pr.poses[1, 9:])
    Jx, Jp = gm.jacobians(pr)
    Bf = gm.free_basis(pr, norm1)
    n, h = Bf.shape[1], 1e-6
    for k in range(n):
        e = np.zeros(n)
        e[k] = h
        numeric = (residual_vector(retract(pr, norm1, e)) - residual_vector(retract(pr, norm1, -e))) / (2 * h)
        analytic = np.zeros((pr.M, 2))
        for f in range(1, pr.F):
            col = Bf[6 * (f - 1):6 * f, k]
            analytic[pr.ofr == f] = Jp[pr.ofr == f] @ col
        assert np.abs(numeric - analytic.reshape(-1)).max() <= 1e-6 * max(1.0, np.abs(analytic).max()), k
    for l in range(pr.L):
        for c in range(3):
            d = np.zeros_like(pr.X)
            d[l, c] = h
            numeric = (residual_vector(pr.with_state(pr.poses, pr.X + d)) - residual_vector(pr.with_state(pr.poses, pr.X - d))) / (2 * h)
            analytic = np.zeros((pr.M, 2))
            analytic[pr.obl == l] = Jx[pr.obl == l][:, :, c]
            assert np.abs(numeric - analytic.reshape(-1)).max() <= 1e-6 * max(1.0, np.abs(analytic).max()), (l, c)
    # |t_1| is held by the retraction
    moved = retract(pr, norm1, 0.05 * rng.standard_normal(n))
    assert abs(np.linalg.norm(moved.poses[1, 9:]) - norm1) <= 4e-16 * norm1
    R = moved.poses[:, :9].reshape(-1, 3, 3)
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-14


@pytest.mark.parametrize("lam", [1e-4, 1e-1, 10.0])
def test_schur_step_equals_the_dense_solve(lam):
    truth, rng = gm.make_scene(F=4, L=25, seed=2, noise=0.5, outliers=0.2)
    pr = gm.perturb(truth, rng)
    norm1 = np.linalg.norm(pr.poses[1, 9:])
    lin = gm.linearise(pr)
    H, g, _ = gm.reduced_system(pr, lin, lam, norm1)
    x = gm.cholesky_solve(H, g)
    st = gm.apply_step(pr, lin, lam, norm1, x)
    # the whole Jacobian over (reduced pose unknowns, landmarks), the damped normal equations, one dense solve
    Bf = gm.free_basis(pr, norm1)
    n = Bf.shape[1]
    J = np.zeros((2 * pr.M, n + 3 * pr.L))
    for o in range(pr.M):
        f, l = pr.ofr[o], pr.obl[o]
        if f >= 1:
            J[2 * o:2 * o + 2, :n] = lin["Jp"][o] @ Bf[6 * (f - 1):6 * f]
        J[2 * o:2 * o + 2, n + 3 * l:n + 3 * l + 3] = lin["Jx"][o]
    w = np.repeat(lin["w"], 2)
    Hd = J.T @ (w[:, None] * J)
    bd = J.T @ (w * lin["r"].reshape(-1))
    dense = np.linalg.solve(Hd + lam * np.diag(np.diag(Hd)), -bd)
    scale = np.abs(dense).max()
    assert np.abs(dense[:n] - x).max() <= 1e-9 * scale
    assert np.abs(dense[n:].reshape(-1, 3) - st["dl"]).max() <= 1e-9 * scale
    assert np.isclose(st["step_sq"], dense @ dense, rtol=1e-9)


def test_a_landmark_without_information_takes_no_step():
    truth, rng = gm.make_scene(F=3, L=10, seed=3)
    pr = gm.perturb(truth, rng)
    X = pr.X.copy()
    X[4] = [0.0, 0.0, -5.0]                  # behind every camera: all of its observations are invalid
    pr = pr.with_state(pr.poses, X)
    lin = gm.linearise(pr)
    assert not lin["valid"][pr.obl == 4].any() and not lin["Hll"][4].any()
    norm1 = np.linalg.norm(pr.poses[1, 9:])
    H, g, extra = gm.reduced_system(pr, lin, 1e-4, norm1)
    assert not extra["alive"][4] and extra["alive"].sum() == 9
    st = gm.apply_step(pr, lin, 1e-4, norm1, gm.cholesky_solve(H, g))
    assert not st["dl"][4].any() and st["dl"].any()


def gauge_distance(result, truth):
    return max(np.abs(result.poses - truth.poses).max(), np.abs(result.X - truth.X).max())


@pytest.mark.parametrize("F,L,seed", [(2, 30, 4), (3, 40, 5), (6, 60, 6)])
def test_noise_free_scene_returns_the_ground_truth(F, L, seed):
    """frame 0 and |t_1| of the start are the truth's, so the minimiser is the truth itself, not a similar copy of it"""
    truth, rng = gm.make_scene(F=F, L=L, seed=seed)
    start = gm.perturb(truth, rng)
    assert np.array_equal(start.poses[0], truth.poses[0])
    assert abs(np.linalg.norm(start.poses[1, 9:]) - np.linalg.norm(truth.poses[1, 9:])) <= 1e-15
    assert gauge_distance(start, truth) > 1e-2
    out = gm.solve(start, ftol=0.0, ptol=1e-24, max_iterations=40)
    assert out["final_cost"] <= 1e-18 * out["initial_cost"]
    assert gauge_distance(out["problem"], truth) <= 1e-9
    # and at the reference's tolerances the run ends by them
    out = gm.solve(start)
    assert out["converged"] and out["iterations"] < 20 and gauge_distance(out["problem"], truth) <= 1e-4


def robust_cost_in_the_chart(pr, norm1, z):
    n = 6 * (pr.F - 1) - 1
    moved = retract(pr, norm1, z[:n])
    return float(gm.evaluate(moved.with_state(moved.poses, moved.X + z[n:].reshape(-1, 3)))["cost"])


def test_stationary_among_gross_outliers():
    from scipy.optimize import minimize
    truth, rng = gm.make_scene(F=6, L=30, seed=25, noise=0.3, outliers=0.3, min_obs=4)
    start = gm.perturb(truth, rng)
    out = gm.solve(start, ftol=1e-14, ptol=1e-20, max_iterations=400)
    pr = out["problem"]
    norm1 = np.linalg.norm(pr.poses[1, 9:])
    lin = gm.linearise(pr)
    # (the cost jumps where an observation turns invalid, and a run can come to rest against such a jump: this one does not)
    assert out["nvalid"] == pr.M and out["converged"]
    assert (lin["w"][lin["valid"]] < 1.0).mean() > 0.15           # the outliers are there and carry Huber weights
    # the tangent-space gradient of the robust cost: J^T w r over the reduced pose unknowns and the landmarks
    Bf = gm.free_basis(pr, norm1)
    gp = Bf.T @ lin["bp"].reshape(-1)[6:]
    gl = lin["bl"].reshape(-1)
    # |g_i| <= sqrt(H_ii sum w r^2) by Cauchy-Schwarz: "vanishes" is 1e-6 of that bound
    _, _, extra = gm.reduced_system(pr, lin, 0.0, norm1)
    bound_p = 1e-6 * np.sqrt(np.diag(extra["Hm"]) * 2 * out["final_cost"])
    bound_l = 1e-6 * np.sqrt(np.stack([lin["Hll"][:, i, i] for i in range(3)], -1) * 2 * out["final_cost"]).reshape(-1)
    assert np.all(np.abs(gp) <= bound_p) and np.all(np.abs(gl) <= bound_l)
    # a general-purpose minimiser started there finds nothing lower
    n = Bf.shape[1] + 3 * pr.L
    res = minimize(lambda z: robust_cost_in_the_chart(pr, norm1, z), np.zeros(n), method="L-BFGS-B", options={"maxiter": 3})
    assert res.fun >= out["final_cost"] * (1 - 1e-9), (res.fun, out["final_cost"])


def test_triangulation_returns_exact_points_from_exact_bearings():
    truth, _ = gm.make_scene(F=8, L=50, seed=7, min_obs=2)
    has = np.zeros(truth.L, np.uint8)
    has[::5] = 1
    given = np.where(has[:, None].astype(bool), np.full((truth.L, 3), 123.0), np.nan)
    pr = truth.with_state(truth.poses, given)
    counts = np.diff(truth.off)
    run, X, vals = gm.triangulate(pr, has, 4, False)
    assert np.array_equal(run, (has == 0) & (counts > 4)) and (counts == 4).any() and run.any()
    assert np.abs(X[run] - truth.X[run]).max() <= 1e-9
    assert np.array_equal(X[~run], given[~run], equal_nan=True)
    assert np.all(vals[run, 0] <= 1e-12 * vals[run, 3])
    run_all, X_all, _ = gm.triangulate(pr, has, 2, True)
    assert np.array_equal(run_all, counts > 2) and np.abs(X_all[run_all] - truth.X[run_all]).max() <= 1e-8


def test_pruning_rule():
    truth, _ = gm.make_scene(F=3, L=20, seed=8)
    oxy = truth.oxy.copy()
    oxy[0] += [0.5, 0.0]        # exactly at the threshold only up to the rounding of q: decided by the strict comparison of the sum
    oxy[1] += [0.6, 0.0]
    oxy[2] += [0.3, 0.3]
    X = truth.X.copy()
    X[-1] = [0.0, 0.0, -1.0]
    pr = gm.Problem(truth.cam, truth.poses, X, truth.off, truth.ofr, oxy)
    flags = gm.flag_outliers(pr)
    assert flags[1] and not flags[2] and flags[pr.obl == truth.L - 1].all()
    assert not flags[3:truth.off[-2]].any()
    assert np.array_equal(gm.flag_outliers(pr, 0.7)[:3], [False, False, False])


def test_track_composition():
    track = gm.make_track()
    frames, landmarks, records = gm.run_bootstrap(gm.ModelBackend(), track)
    assert [r["iterations"] > 0 for r in records] == [True] * 3 and all(r["final_cost"] < r["initial_cost"] for r in records)
    assert sum(r["triangulated"] for r in records) > 0 and all(r["removed"] > 0 for r in records)
    # the uninitialised frame keeps its pose; frame 0 of every window is fixed; the others moved
    before = track[1]
    assert np.array_equal(frames[2]["t_world_agent"], before[2]["t_world_agent"]) and not before[2]["initialized"]
    assert np.abs(frames[0]["t_world_agent"] - before[0]["t_world_agent"]).max() <= 1e-15
    assert all(np.abs(frames[i]["t_world_agent"] - before[i]["t_world_agent"]).max() > 1e-6 for i in (1, 3, 4, 5))
    assert sum(lm["has"] for lm in landmarks) == sum(lm["has"] for lm in track[2]) + sum(r["triangulated"] for r in records)
    assert sum(len(lm["proj"]) for lm in track[2]) - sum(len(lm["proj"]) for lm in landmarks) == sum(r["removed"] for r in records)


def test_no_cpu_fallback():
    from dsopp_amd import capi
    if capi.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(capi.HipError) as e:
        capi.GeometricBA()
    assert "no HIP device" in str(e.value) or "-4" in str(e.value)


def build_example(tmp_path):
    libdir = os.path.join(ROOT, "dsopp_amd", "lib")
    exe = str(tmp_path / "example_refine_track")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "dsopp_amd", "host", "example_refine_track.cpp"),
                           f"-L{libdir}", "-ldsopp_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", exe])
    return exe


def test_example_driver_compiles_and_fails_loudly_without_gpu(tmp_path):
    from dsopp_amd import capi
    exe = build_example(tmp_path)
    if capi.device_count() > 0:
        pytest.skip("GPU present: tests/test_gpu_geometric_ba.py runs it")
    r = subprocess.run([exe, "/nonexistent"], capture_output=True, text=True)
    assert r.returncode == 2 and "no CPU fallback" in r.stdout
