"""The NumPy statement of the geometric bundle adjustment's camera block (include/dsopp_hip.h, dsopp_hip_geometric_ba_evaluate_camera and
_solve_camera): the camera's intrinsics as a third parameter block beside poses and landmarks, for a pinhole (fx, fy, cx, cy) or a
simple-radial (f, cx, cy, k1, k2) camera, with ParameterParameterization's five fix flags.  Everything the camera block shares with the
solver without it — the pose algebra, the Huber weights, the landmark factor, the reduced pose system, the Cholesky — is
tests/geometric_ba_model.py's, called, not copied: with every intrinsic fixed a pinhole run IS gm.solve's run.  Every function takes a
`dtype` like the model it extends.  max_valid_radius is tests/camera_remap_model.py's simple_radial_derived, in binary64 whatever the
dtype: it enters a comparison only.

A problem is gm's Problem, of whose cam only width and height (cam[4], cam[5]) are read; the camera is a Camera."""
import dataclasses

import numpy as np

import camera_remap_model as crm
import geometric_ba_model as gm

PINHOLE, SIMPLE_RADIAL = 0, 1
FIX_FOCAL, FIX_CENTER, FIX_MODEL_SPECIFIC, FIX_POSES, FIX_LANDMARKS = 1, 2, 4, 8, 16
GROUPS = {PINHOLE: (FIX_FOCAL, FIX_FOCAL, FIX_CENTER, FIX_CENTER),
          SIMPLE_RADIAL: (FIX_FOCAL, FIX_CENTER, FIX_CENTER, FIX_MODEL_SPECIFIC, FIX_MODEL_SPECIFIC)}
NC = 5     # the columns every camera quantity carries; a pinhole's fifth is zero


@dataclasses.dataclass
class Camera:
    model: int
    c: np.ndarray           # the intrinsics, 4 or 5
    fixed: int = 0

    def __post_init__(self):
        self.c = np.array(self.c)
        assert len(self.c) == len(GROUPS[self.model]), self.c

    def with_intrinsics(self, c):
        return Camera(self.model, np.array(c), self.fixed)


def free_intrinsics(model, fixed):
    """constantParameterSet's complement: the free intrinsics' indices in parameter order"""
    return [k for k, group in enumerate(GROUPS[model]) if not fixed & group]


def unknowns(model, fixed, F):
    """(pose unknowns, free intrinsics, landmarks move) of the reduced system: the free intrinsics follow the pose unknowns"""
    return (0 if fixed & FIX_POSES else 6 * (F - 1) - 1), free_intrinsics(model, fixed), not fixed & FIX_LANDMARKS


def max_valid_radius(pr, cam):
    """simple radial: the constructor's constant of the camera as it is; 0 for a pinhole"""
    if cam.model == PINHOLE:
        return 0.0
    return float(crm.simple_radial_derived(pr.cam[4], pr.cam[5], *[float(v) for v in cam.c])[0][0])


def camera_is_valid(pr, cam):
    """the rule a candidate camera must pass (and the entry camera, or the call is invalid)"""
    c = np.asarray(cam.c, np.float64)
    if not np.all(np.isfinite(c)) or not c[0] > 0 or (cam.model == PINHOLE and not c[1] > 0):
        return False
    if cam.model == SIMPLE_RADIAL:
        with np.errstate(all="ignore"):
            radius = max_valid_radius(pr, cam)
        return bool(np.isfinite(radius) and radius > 0)
    return True


def as_pinhole(pr, cam):
    """the Problem gm's pinhole functions take"""
    out = pr.with_state(pr.poses, pr.X)
    out.cam = tuple(cam.c[:4]) + tuple(pr.cam[4:])
    return out


def project(pr, cam, dtype=np.float64, radius=None):
    """valid (M,), q (M, 2), pc (M, 3)"""
    if cam.model == PINHOLE:
        return gm.project(as_pinhole(pr, cam), dtype)
    width, height = pr.cam[4], pr.cam[5]
    f, cx, cy, k1, k2 = (dtype(v) for v in cam.c)
    radius = dtype(max_valid_radius(pr, cam) if radius is None else radius)
    R, t = gm.pose_parts(pr.poses.astype(dtype))
    pc = np.einsum("mij,mj->mi", R[pr.ofr], pr.X.astype(dtype)[pr.obl]) + t[pr.ofr]
    with np.errstate(all="ignore"):
        u, v = pc[:, 0] / pc[:, 2], pc[:, 1] / pc[:, 2]
        rho2 = u * u + v * v
        d = (1 + k1 * rho2) + (k2 * rho2) * rho2
        q = np.stack([f * (d * u) + cx, f * (d * v) + cy], -1)
        inside = (q[:, 0] >= gm.BORDER) & (q[:, 0] <= width - 1 - gm.BORDER) & (q[:, 1] >= gm.BORDER) & (q[:, 1] <= height - 1 - gm.BORDER)
        valid = (np.sqrt(rho2) <= radius) & inside
    return valid, q, pc


def decision_margins(pr, cam):
    """per observation the distance of its validity decision from flipping, float64: (depth or radius margin, ROI margin); the ROI margin
    is infinite where the first test already fails"""
    valid, q, pc = project(pr, cam)
    width, height = pr.cam[4], pr.cam[5]
    with np.errstate(all="ignore"):
        edge = np.minimum.reduce([np.abs(q[:, 0] - gm.BORDER), np.abs(q[:, 0] - (width - 1 - gm.BORDER)), np.abs(q[:, 1] - gm.BORDER),
                                  np.abs(q[:, 1] - (height - 1 - gm.BORDER))])
        if cam.model == PINHOLE:
            first, passed = np.abs(pc[:, 2] - gm.MIN_DEPTH), pc[:, 2] >= gm.MIN_DEPTH
        else:
            rho = np.sqrt((pc[:, 0] / pc[:, 2]) ** 2 + (pc[:, 1] / pc[:, 2]) ** 2)
            radius = max_valid_radius(pr, cam)
            first, passed = np.abs(rho - radius), rho <= radius
    return first, np.where(passed, edge, np.inf)


def evaluate(pr, cam, a=gm.A_HUBER, dtype=np.float64):
    """dict: valid, r (0 where invalid), w (0 where invalid), cost, nvalid"""
    if cam.model == PINHOLE:
        return gm.evaluate(as_pinhole(pr, cam), a, dtype)
    valid, q, _ = project(pr, cam, dtype)
    r = np.where(valid[:, None], pr.oxy.astype(dtype) - np.where(valid[:, None], q, 0), 0)
    w, rho = gm.huber(np.sum(r * r, -1), dtype(a))
    w = np.where(valid, w, 0)
    return {"valid": valid, "r": r, "w": w, "cost": dtype(0.5) * np.sum(np.where(valid, rho, 0)), "nvalid": int(valid.sum())}


def radial_projection_jacobian(pc, c, dtype=np.float64):
    """G = dq / dp (M, 2, 3) as simple_radial.hpp:190-199 writes it, and (u, v, rho2, d)"""
    f, _, _, k1, k2 = (dtype(v) for v in c)
    x, y, z = pc[:, 0], pc[:, 1], pc[:, 2]
    u, v = x / z, y / z
    rho2 = u * u + v * v
    d = (1 + k1 * rho2) + (k2 * rho2) * rho2
    common = (2 * k1 + 4 * k2 * rho2) / z / z
    last = -3 * k1 * rho2 - 5 * k2 * rho2 * rho2 - 1
    G = np.zeros((len(pc), 2, 3), dtype)
    G[:, 0, 0] = f * (x * x * common + d) / z
    G[:, 0, 1] = G[:, 1, 0] = f * x * y * common / z
    G[:, 1, 1] = f * (y * y * common + d) / z
    G[:, 0, 2] = f * x / z / z * last
    G[:, 1, 2] = f * y / z / z * last
    return G, (u, v, rho2, d)


def jacobians(pr, cam, dtype=np.float64):
    """J_x (M, 2, 3), J_p (M, 2, 6) and J_c = dr / dc (M, 2, 5) of r = obs - q, zero where invalid"""
    Jc = np.zeros((pr.M, 2, NC), dtype)
    if cam.model == PINHOLE:
        prc = as_pinhole(pr, cam)
        Jx, Jp = gm.jacobians(prc, dtype)
        valid, _, pc = gm.project(prc, dtype)
        z = np.where(valid, pc[:, 2], 1)
        Jc[:, 0, 0], Jc[:, 1, 1] = -(pc[:, 0] / z), -(pc[:, 1] / z)
        Jc[:, 0, 2] = Jc[:, 1, 3] = -1
        return Jx, Jp, Jc * valid[:, None, None]
    valid, _, pc = project(pr, cam, dtype)
    pcs = np.where(valid[:, None], pc, 1)
    G, (u, v, rho2, d) = radial_projection_jacobian(pcs, cam.c, dtype)
    R, _ = gm.pose_parts(pr.poses.astype(dtype))
    Jx = -np.einsum("mij,mjk->mik", G, R[pr.ofr]) * valid[:, None, None]
    A = np.concatenate([np.broadcast_to(np.eye(3, dtype=dtype), (pr.L, 3, 3)), -gm.hat(pr.X.astype(dtype))], -1)
    f = dtype(cam.c[0])
    f2, f4 = f * rho2, f * (rho2 * rho2)
    Jc[:, 0, 0], Jc[:, 1, 0] = -(d * u), -(d * v)
    Jc[:, 0, 1] = Jc[:, 1, 2] = -1
    Jc[:, 0, 3], Jc[:, 1, 3] = -(f2 * u), -(f2 * v)
    Jc[:, 0, 4], Jc[:, 1, 4] = -(f4 * u), -(f4 * v)
    return Jx, np.einsum("mij,mjk->mik", Jx, A[pr.obl]), Jc * valid[:, None, None]


def linearise(pr, cam, a=gm.A_HUBER, dtype=np.float64):
    """gm.linearise's dict and the camera's blocks over all five columns: Jc, Wc (M, 3, 5) = w J_x^T J_c, Wlc (L, 3, 5) its sum per
    landmark, Hpc (F, 6, 5), Hcc (5, 5), bc (5,)"""
    if cam.model == PINHOLE:
        lin = gm.linearise(as_pinhole(pr, cam), a, dtype)
        Jx, Jp, Jc = jacobians(pr, cam, dtype)
    else:
        ev = evaluate(pr, cam, a, dtype)
        Jx, Jp, Jc = jacobians(pr, cam, dtype)
        w, r = ev["w"], ev["r"]
        F, L = pr.F, pr.L
        C = np.einsum("m,mki,mkj->mij", w, Jx, Jx)
        c = np.einsum("m,mki,mk->mi", w, Jx, r)
        Hll, bl = np.zeros((L, 3, 3), dtype), np.zeros((L, 3), dtype)
        np.add.at(Hll, pr.obl, C)
        np.add.at(bl, pr.obl, c)
        Hpp, bp = np.zeros((F, 6, 6), dtype), np.zeros((F, 6), dtype)
        np.add.at(Hpp, pr.ofr, np.einsum("m,mki,mkj->mij", w, Jp, Jp))
        np.add.at(bp, pr.ofr, np.einsum("m,mki,mk->mi", w, Jp, r))
        W = np.einsum("m,mki,mkj->mij", w, Jp, Jx)
        lin = dict(ev, Jx=Jx, Jp=Jp, C=C, c=c, Hll=Hll, bl=bl, Hpp=Hpp, bp=bp, W=W)
    w, r = lin["w"], lin["r"]
    Wc = np.einsum("m,mki,mkj->mij", w, Jx, Jc)
    Wlc = np.zeros((pr.L, 3, NC), dtype)
    np.add.at(Wlc, pr.obl, Wc)
    Hpc = np.zeros((pr.F, 6, NC), dtype)
    np.add.at(Hpc, pr.ofr, np.einsum("m,mki,mkj->mij", w, Jp, Jc))
    return dict(lin, Jc=Jc, Wc=Wc, Wlc=Wlc, Hpc=Hpc, Hcc=np.einsum("m,mki,mkj->ij", w, Jc, Jc), bc=np.einsum("m,mki,mk->i", w, Jc, r))


def _eliminated(lin, moves):
    """the linearisation the pose system sees: with fixed landmarks H_ll = 0, so that no landmark is eliminated and S = 0"""
    return lin if moves else dict(lin, Hll=np.zeros_like(lin["Hll"]))


def reduced_system(pr, cam, lin, lam, norm1, dtype=np.float64):
    """(H (n, n) damped, g (n,), extras): gm's reduced pose system bordered by the free intrinsics' rows and columns.  extras: diag =
    the undamped diagonal of B^T H B (what was added into every entry), alive, Li, Bf (None with fixed poses)"""
    npose, free, moves = unknowns(cam.model, cam.fixed, pr.F)
    lam = dtype(lam)
    seen = _eliminated(lin, moves)
    alive, Li = gm.landmark_factor(seen["Hll"], lam)
    Yc = np.einsum("lij,ljk->lik", Li, lin["Wlc"])[:, :, free]                    # L^-1 W_lc, zero for a dead landmark
    z = np.einsum("lij,lj->li", Li, lin["bl"])
    Hcc = lin["Hcc"][np.ix_(free, free)]
    Scc = np.einsum("lki,lkj->ij", Yc, Yc)
    Hc = Hcc - Scc + lam * np.diag(np.diag(Hcc))
    gc = -(lin["bc"][free] - np.einsum("lki,lk->i", Yc, z))
    if npose == 0:
        return Hc, gc, dict(diag=np.diag(Hcc).copy(), alive=alive, Li=Li, Bf=None)
    Hp, gp, extra = gm.reduced_system(pr, seen, lam, norm1, dtype)
    Bf = extra["Bf"]
    Y = np.einsum("mij,mkj->mik", Li[pr.obl], lin["W"])                           # (M, 3, 6), as gm has it
    Spc = np.zeros((pr.F, 6, len(free)), dtype)
    np.add.at(Spc, pr.ofr, np.einsum("mki,mkj->mij", Y, Yc[pr.obl]))
    Hpc = Bf.T @ (lin["Hpc"][1:, :, free] - Spc[1:]).reshape(6 * (pr.F - 1), len(free))
    H = np.block([[Hp, Hpc], [Hpc.T, Hc]])
    return H, np.concatenate([gp, gc]), dict(diag=np.concatenate([np.diag(extra["Hm"]), np.diag(Hcc)]), alive=alive, Li=Li, Bf=Bf)


def apply_step(pr, cam, lin, lam, norm1, x, a=gm.A_HUBER, dtype=np.float64):
    """the rest of an iteration for the step x (pose unknowns, then the free intrinsics): back-substitution, retraction, the candidate
    state and camera, its cost; camera_ok = the candidate camera passes camera_is_valid"""
    F = pr.F
    npose, free, moves = unknowns(cam.model, cam.fixed, F)
    x = np.asarray(x, dtype)
    lam = dtype(lam)
    dc = np.zeros(NC, dtype)
    dc[free] = x[npose:]
    d6 = np.zeros((F, 6), dtype)
    R, t = gm.pose_parts(pr.poses.astype(dtype))
    cand = pr.poses.astype(dtype).copy()
    if npose:
        B, b1, b2 = gm.frame1_basis(pr, norm1, dtype)
        d6[1] = B @ x[:5]
        d6[2:] = x[5:npose].reshape(F - 2, 6)
        E1, _ = gm.exp_se3(np.concatenate([np.zeros(3, dtype), d6[1, 3:]]), dtype)
        cand[1, :9] = (R[1] @ E1).reshape(9)
        vdir = t[1] / np.sqrt(t[1] @ t[1]) + x[0] * b1 + x[1] * b2
        cand[1, 9:] = dtype(norm1) * (vdir / np.sqrt(vdir @ vdir))
        for f in range(2, F):
            E, et = gm.exp_se3(d6[f], dtype)
            cand[f, :9] = (R[f] @ E).reshape(9)
            cand[f, 9:] = R[f] @ et + t[f]
    X = pr.X.astype(dtype)
    dl = np.zeros_like(X)
    if moves:
        alive, Li = gm.landmark_factor(lin["Hll"], lam)
        u = d6[pr.ofr, :3] + np.cross(d6[pr.ofr, 3:], X[pr.obl])
        v = lin["bl"].copy()
        np.add.at(v, pr.obl, np.einsum("mij,mj->mi", lin["C"], u))
        if free:
            v = v + np.einsum("lij,j->li", lin["Wlc"], dc)
        y = np.einsum("lij,lj->li", Li, v)
        dl = -np.einsum("lji,lj->li", Li, y)
    candidate = pr.with_state(cand, X + dl)
    candidate.cam = pr.cam
    camera = cam.with_intrinsics(np.asarray(cam.c, dtype) + dc[:len(cam.c)])
    ok = camera_is_valid(pr, camera)
    ev = evaluate(candidate, camera, a, dtype) if ok else dict(cost=dtype(np.inf), nvalid=0)
    step = x @ x + np.sum(dl * dl)
    state = dtype(0)
    if npose:
        state = np.sum(t[1:] * t[1:]) + (F - 1)
    if moves:
        state = state + np.sum(X * X)
    if free:
        state = state + np.sum(np.asarray(cam.c, dtype)[free] ** 2)
    return dict(candidate=candidate, camera=camera, camera_ok=ok, cost=ev["cost"], nvalid=ev["nvalid"], step_sq=step, state_sq=state, dl=dl,
                d6=d6, dc=dc)


def solve(pr, cam, a=gm.A_HUBER, lambda_0=gm.LAMBDA_0, ftol=gm.FTOL, ptol=gm.PTOL, decrease=gm.DECREASE, increase=gm.INCREASE,
          max_iterations=gm.MAX_ITERATIONS, dtype=np.float64, keep_states=False):
    """gm.solve's driver with the camera among the state.  Returns its dict and camera (the final one); states holds
    (Problem, Camera, lambda)"""
    pr = pr.with_state(pr.poses.astype(dtype), pr.X.astype(dtype))
    cam = cam.with_intrinsics(np.asarray(cam.c, dtype))
    npose, free, moves = unknowns(cam.model, cam.fixed, pr.F)
    assert npose or free or moves, "nothing is free"
    assert camera_is_valid(pr, cam)
    norm1 = None
    if npose:
        t1 = pr.poses[1, 9:]
        norm1 = np.sqrt(t1 @ t1)
    lam = dtype(lambda_0)
    ev = evaluate(pr, cam, a, dtype)
    E, nvalid = ev["cost"], ev["nvalid"]
    out = dict(initial_cost=E, iterations=0, accepted=0, reason=0, trace=[], states=[])
    lin, it = None, 0
    if nvalid == 0:
        out["reason"] = gm.NO_VALID_RESIDUAL
    while it < max_iterations and out["reason"] == 0:
        if lin is None:
            lin = linearise(pr, cam, a, dtype)
        if keep_states:
            out["states"].append((pr, cam, lam))
        H, g, _ = reduced_system(pr, cam, lin, lam, norm1, dtype)
        x = gm.cholesky_solve(H, g)
        it += 1
        st = apply_step(pr, cam, lin, lam, norm1, x, a, dtype) if x is not None else None
        if st is None or not st["camera_ok"]:
            out["trace"].append((E, dtype(np.inf), 0, lam))
            lam = lam * dtype(increase)
            continue
        En = st["cost"]
        if st["nvalid"] == 0:
            out["trace"].append((E, En, 0, lam))
            out["reason"] = gm.NO_VALID_RESIDUAL
            break
        reason = gm.FUNCTION_TOLERANCE if abs(E - En) / E < ftol else 0
        if En < E:
            out["trace"].append((E, En, 1, lam))
            if st["step_sq"] < dtype(ptol) * (st["state_sq"] + dtype(ptol)):
                reason |= gm.PARAMETER_TOLERANCE
            pr, cam, E, nvalid, lin = st["candidate"], st["camera"], En, st["nvalid"], None
            lam = lam / dtype(decrease)
            out["accepted"] += 1
        else:
            out["trace"].append((E, En, 0, lam))
            lam = lam * dtype(increase)
        out["reason"] = reason
    out.update(problem=pr, camera=cam, final_cost=E, nvalid=nvalid, iterations=it, converged=bool(out["reason"] & 3), **{"lambda": lam})
    return out
