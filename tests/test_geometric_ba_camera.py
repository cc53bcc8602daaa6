"""The NumPy statement of the geometric bundle adjustment's camera block (tests/geometric_ba_camera_model.py) pinned on the CPU: its
Jacobians against central differences of its own residual in extended precision, its run with every intrinsic fixed against
geometric_ba_model's, the recovery of a camera that starts off the truth on noise-free scenes, the radius rule, and which unknowns exist
under each combination of the fix flags."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_remap_model as crm
import geometric_ba_camera_model as gc
import geometric_ba_model as gm

K_TRUE = (-0.12, 0.03)
LD = np.longdouble


def radial_scene(F, L, seed, noise=0.0):
    """(truth Problem observed through the simple-radial camera, its intrinsics, rng)"""
    truth, rng = gm.make_scene(F=F, L=L, seed=seed, noise=0.0)
    fx, _, cx, cy = truth.cam[:4]
    c = np.array([fx, cx, cy, K_TRUE[0], K_TRUE[1]])
    valid, q, _ = gc.project(truth, gc.Camera(gc.SIMPLE_RADIAL, c))
    assert valid.all()
    return gm.Problem(truth.cam, truth.poses, truth.X, truth.off, truth.ofr, q + noise * rng.standard_normal(q.shape)), c, rng


# ---- the Jacobians

def projections(pr, cam, pc=None):
    """q (M, 2) in longdouble, without the validity rule: of the problem's observations, or of given camera-frame points"""
    if pc is None:
        R, t = gm.pose_parts(pr.poses.astype(LD))
        pc = np.einsum("mij,mj->mi", R[pr.ofr], pr.X.astype(LD)[pr.obl]) + t[pr.ofr]
    c = np.asarray(cam.c, LD)
    u, v = pc[:, 0] / pc[:, 2], pc[:, 1] / pc[:, 2]
    if cam.model == gc.PINHOLE:
        return np.stack([c[0] * u + c[2], c[1] * v + c[3]], -1), pc
    rho2 = u * u + v * v
    d = (1 + c[3] * rho2) + (c[4] * rho2) * rho2
    return np.stack([c[0] * (d * u) + c[1], c[0] * (d * v) + c[2]], -1), pc


@pytest.mark.parametrize("model", [gc.PINHOLE, gc.SIMPLE_RADIAL])
def test_camera_jacobian_against_central_differences(model):
    """r = obs - q is linear in each single intrinsic (q = f d (u, v) + centre is a product of f, of d which is linear in k1 and k2, and
    a sum with the centre), so a central difference in one intrinsic has no truncation error at all: what is left is the rounding of two
    longdouble evaluations of q, each a handful of operations, divided by 2 h.  Bar: 64 eps_longdouble max|q| / h with h = 1e-4 relative to
    1 + |c_i|; about 4e-11 on entries of up to 200."""
    pr, c, rng = radial_scene(3, 63, 4)
    if model == gc.PINHOLE:
        c = np.array(pr.cam[:4])
    c = c * (1 + 0.01 * rng.standard_normal(len(c)))
    cam = gc.Camera(model, c)
    valid, _, _ = gc.project(pr, cam)
    assert valid.all()
    _, _, Jc = gc.jacobians(pr, cam, LD)
    q0, _ = projections(pr, cam)
    eps = float(np.finfo(LD).eps)
    worst = 0.0
    for k in range(len(c)):
        h = LD(1e-4) * (1 + abs(LD(c[k])))
        up, down = np.asarray(c, LD).copy(), np.asarray(c, LD).copy()
        up[k] += h
        down[k] -= h
        diff = -(projections(pr, cam.with_intrinsics(up))[0] - projections(pr, cam.with_intrinsics(down))[0]) / (2 * h)
        bar = 64 * eps * float(np.abs(q0).max()) / float(h)
        err = float(np.abs(diff - Jc[:, :, k]).max())
        worst = max(worst, err / bar)
        assert err <= bar, (k, err, bar)
    assert np.all(Jc[:, :, len(c):] == 0)
    print(f"model {model}: worst J_c error {worst:.3e} of its bar")


def test_simple_radial_projection_jacobian_against_central_differences():
    """G = dq / dp as simple_radial.hpp:190-199 writes it.  q is homogeneous of degree 0 in p, its third derivatives of degree -3:
    |d3 q| <= K f / p_z^3, where the pinhole's x / z contributes 6 |u| and the distortion polynomial (degree 5 in (u, v), |k1| <= 0.13,
    |k2| <= 0.04, rho <= 0.8 on this scene) multiplies that by less than 16: K = 100 is generous.  Central difference with step h:
    truncation h^2 / 6 * K f / z_min^3, rounding 64 eps_longdouble max|q| / h.  With h = 1e-6 the bar is about 1e-10 on entries of the
    order of f / z = 80."""
    pr, c, rng = radial_scene(3, 63, 4)
    c = c * (1 + 0.01 * rng.standard_normal(5))
    cam = gc.Camera(gc.SIMPLE_RADIAL, c)
    q0, pc = projections(pr, cam)
    assert np.sqrt(((pc[:, :2] / pc[:, 2:]) ** 2).sum(-1)).max() <= 0.8
    G, _ = gc.radial_projection_jacobian(pc, c, LD)
    h = LD(1e-6)
    eps = float(np.finfo(LD).eps)
    bar = float(h) ** 2 / 6 * 100 * c[0] / float(pc[:, 2].min()) ** 3 + 64 * eps * float(np.abs(q0).max()) / float(h)
    for k in range(3):
        up, down = pc.copy(), pc.copy()
        up[:, k] += h
        down[:, k] -= h
        diff = (projections(pr, cam, up)[0] - projections(pr, cam, down)[0]) / (2 * h)
        err = float(np.abs(diff - G[:, :, k]).max())
        print(f"dq / dp_{k}: error {err:.3e}, bar {bar:.3e}")
        assert err <= bar
    # and the Jacobians the solver takes are -G R and -G R [I | -hat(X)]
    Jx, Jp, _ = gc.jacobians(pr, cam, LD)
    R, _ = gm.pose_parts(pr.poses.astype(LD))
    assert np.abs(Jx + np.einsum("mij,mjk->mik", G, R[pr.ofr])).max() <= 1e-15
    assert np.abs(Jp[:, :, :3] - Jx).max() == 0


# ---- every intrinsic fixed

@pytest.mark.parametrize("F,L,seed,outliers", [(2, 40, 3, 0.0), (3, 63, 4, 0.0), (5, 120, 22, 0.3)])
def test_every_intrinsic_fixed_is_the_model_without_a_camera_block(F, L, seed, outliers):
    truth, rng = gm.make_scene(F=F, L=L, seed=seed, noise=0.3, outliers=outliers)
    start = gm.perturb(truth, rng)
    a = gm.solve(start, keep_states=True)
    b = gc.solve(start, gc.Camera(gc.PINHOLE, start.cam[:4], gc.FIX_FOCAL | gc.FIX_CENTER | gc.FIX_MODEL_SPECIFIC), keep_states=True)
    assert a["iterations"] == b["iterations"] > 1 and a["trace"] == b["trace"] and a["reason"] == b["reason"]
    assert np.array_equal(a["problem"].poses, b["problem"].poses) and np.array_equal(a["problem"].X, b["problem"].X)
    assert a["final_cost"] == b["final_cost"] and a["lambda"] == b["lambda"] and np.array_equal(b["camera"].c, start.cam[:4])
    for (pa, la), (pb, _, lb) in zip(a["states"], b["states"]):
        assert la == lb and np.array_equal(pa.poses, pb.poses) and np.array_equal(pa.X, pb.X)


# ---- a camera that starts off the truth

@pytest.mark.parametrize("F,L,seed", [(3, 63, 4), (5, 120, 22)])
@pytest.mark.parametrize("model", [gc.PINHOLE, gc.SIMPLE_RADIAL])
def test_free_intrinsics_move_towards_the_truth(F, L, seed, model):
    """noise-free observations, the state at the truth, the camera off it: focal +3 % / -3 %, centre +6 / -4 px, k1 = k2 = 0 against
    -0.12 / 0.03.  Every intrinsic ends closer to the truth than it began; the distances are printed, not fixed in advance."""
    if model == gc.PINHOLE:
        pr, _ = gm.make_scene(F=F, L=L, seed=seed, noise=0.0)
        true_c = np.array(pr.cam[:4])
        start_c = true_c * [1.03, 0.97, 1.0, 1.0] + [0.0, 0.0, 6.0, -4.0]
    else:
        pr, true_c, _ = radial_scene(F, L, seed)
        start_c = np.array([true_c[0] * 1.03, true_c[1] + 6.0, true_c[2] - 4.0, 0.0, 0.0])
    out = gc.solve(pr, gc.Camera(model, start_c))
    before, after = np.abs(start_c - true_c), np.abs(out["camera"].c - true_c)
    print(f"F{F}_L{L} model {model}: {out['iterations']} iterations, reason {out['reason']}, cost {out['initial_cost']:.3e} -> {out['final_cost']:.3e}")
    print(f"  distance to the truth before {before}, after {after}")
    assert np.all(after < before), (before, after)
    assert out["accepted"] > 0 and out["final_cost"] < out["initial_cost"]


# ---- the radius rule

def test_a_point_is_valid_up_to_the_radius():
    """frame 0 is the identity, so rho = X_x of a point on the x axis at depth 1; the radius is camera_remap_model's"""
    for c in ([128.0, 128.0, 128.0, -0.6, 0.05], [200.0, 160.0, 120.0, -0.5, 0.04]):
        shape = (0.0, 0.0, 0.0, 0.0, 2048, 2048)          # wide enough that no q of these points leaves the ROI
        derived, replaced = crm.simple_radial_derived(2048, 2048, *c)   # the extremum rule: beyond it the projection would fold back
        radius = float(derived[0])
        assert replaced
        cam = gc.Camera(gc.SIMPLE_RADIAL, c)
        poses = np.zeros((1, 12))
        poses[0, [0, 4, 8]] = 1.0
        X = np.array([[radius, 0.0, 1.0], [np.nextafter(radius, 0.0), 0.0, 1.0], [np.nextafter(radius, 9.0), 0.0, 1.0],
                      [-radius, 0.0, -1.0], [radius * (1 + 1e-9), 0.0, 1.0], [0.6 * radius, -0.8 * radius * (1 - 1e-9), 1.0]])
        pr = gm.Problem(shape, poses, X, np.arange(7), np.zeros(6, np.int32), np.zeros((6, 2)))
        assert gc.max_valid_radius(pr, cam) == radius
        valid, q, _ = gc.project(pr, cam)
        assert valid.tolist() == [True, True, False, True, False, True], (c, valid)
        ev = gc.evaluate(pr, cam)
        assert np.all(ev["r"][~valid] == 0) and np.all(ev["w"][~valid] == 0) and ev["nvalid"] == 4
        _, _, Jc = gc.jacobians(pr, cam)
        assert np.all(Jc[~valid] == 0) and np.all(Jc[valid][:, 0, 1] == -1)
    # no derivative flows through the radius: the candidate's validity is decided with the candidate camera's own radius
    moved = gc.Camera(gc.SIMPLE_RADIAL, [128.0, 128.0, 128.0, -0.5, 0.05])
    assert gc.max_valid_radius(pr, moved) != gc.max_valid_radius(pr, gc.Camera(gc.SIMPLE_RADIAL, [128.0, 128.0, 128.0, -0.6, 0.05]))


# ---- the fix flags

EXPECTED_FREE = {gc.PINHOLE: {gc.FIX_FOCAL: [0, 1], gc.FIX_CENTER: [2, 3], gc.FIX_MODEL_SPECIFIC: []},
                 gc.SIMPLE_RADIAL: {gc.FIX_FOCAL: [0], gc.FIX_CENTER: [1, 2], gc.FIX_MODEL_SPECIFIC: [3, 4]}}


@pytest.mark.parametrize("model", [gc.PINHOLE, gc.SIMPLE_RADIAL])
def test_which_unknowns_exist_under_every_combination_of_the_flags(model):
    """2 models x 8 intrinsics combinations x 4 of (poses, landmarks): the size and order of the reduced system, and that one iteration
    moves exactly what is free"""
    truth, rng = gm.make_scene(F=3, L=20, seed=11, noise=0.3)
    start = gm.perturb(truth, rng)
    c0 = np.array(start.cam[:4]) * 1.01 if model == gc.PINHOLE else np.array([323.0, 321.0, 238.0, 0.01, 0.0])
    norm1 = np.linalg.norm(start.poses[1, 9:])
    seen = 0
    for bits in itertools.product((0, 1), repeat=5):
        fixed = sum(b << k for k, b in enumerate(bits))
        npose, free, moves = gc.unknowns(model, fixed, start.F)
        want = sorted(k for group, ks in EXPECTED_FREE[model].items() if not fixed & group for k in ks)
        assert free == want and npose == (0 if fixed & gc.FIX_POSES else 6 * (start.F - 1) - 1) and moves == (not fixed & gc.FIX_LANDMARKS)
        cam = gc.Camera(model, c0, fixed)
        if not (npose or free or moves):
            with pytest.raises(AssertionError):
                gc.solve(start, cam, max_iterations=1)
            continue
        seen += 1
        lin = gc.linearise(start, cam)
        H, g, extra = gc.reduced_system(start, cam, lin, gm.LAMBDA_0, norm1)
        n = npose + len(free)
        assert H.shape == (n, n) and g.shape == (n,) and extra["diag"].shape == (n,) and np.array_equal(H[npose:, :npose], H[:npose, npose:].T)
        # the camera's rows are the free intrinsics in parameter order: the damped diagonal is (1 + lambda) H_cc less the Schur part
        full = gc.reduced_system(start, gc.Camera(model, c0, fixed & (gc.FIX_POSES | gc.FIX_LANDMARKS)), lin, gm.LAMBDA_0, norm1)[0]
        every = gc.free_intrinsics(model, 0)
        rows = list(range(npose)) + [npose + every.index(k) for k in free]
        scale = np.sqrt(extra["diag"])                       # (a product of other shapes may round otherwise: not byte for byte)
        assert np.all(np.abs(H - full[np.ix_(rows, rows)]) <= 1e-12 * np.outer(scale, scale))
        if n == 0:
            x = np.zeros(0)
        else:
            x = gm.cholesky_solve(H, g)
            assert x is not None
        st = gc.apply_step(start, cam, lin, gm.LAMBDA_0, norm1, x)
        moved_c = st["camera"].c != c0
        assert np.all(moved_c[free]) and not np.any(np.delete(moved_c, free))
        assert np.array_equal(st["candidate"].poses[0], start.poses[0])
        assert np.all(np.any(st["candidate"].poses[1:] != start.poses[1:], -1)) == bool(npose) or not npose
        assert (not npose) == np.array_equal(st["candidate"].poses, start.poses)
        assert (not moves) == np.array_equal(st["candidate"].X, start.X)
        norm = (np.sum(np.asarray(c0)[free] ** 2) + (np.sum(start.X ** 2) if moves else 0)
                + (np.sum(start.poses[1:, 9:] ** 2) + start.F - 1 if npose else 0))
        assert abs(st["state_sq"] - norm) <= 1e-12 * norm
        assert abs(st["step_sq"] - (x @ x + np.sum(st["dl"] ** 2))) <= 1e-15 * max(st["step_sq"], 1e-300)
    assert seen == 32 - (2 if model == gc.PINHOLE else 1)
