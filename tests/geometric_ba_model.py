"""The NumPy statement of the bootstrap's geometric bundle adjustment (include/dsopp_hip.h, dsopp_hip_geometric_ba_*): the reprojection
residual with its validity rule, the Huber IRLS blocks, the Schur reduction on the landmarks, the five degrees of freedom of frame 1, the
reference's LM driver, the triangulation and the pruning.  Every function takes a `dtype`: numpy.float64 is the statement, numpy.longdouble
runs the same solve in extended precision (the measure of how far two correct float64 solves may lie apart).  tests/test_geometric_ba.py
pins it on the CPU, tests/test_gpu_geometric_ba.py holds the device to it.

A problem is a Problem: cam = (fx, fy, cx, cy, width, height), poses (F, 12) = R row-major then t of t_agent_world, X (L, 3), off (L + 1),
ofr (M,), oxy (M, 2): the observations grouped by landmark."""
import dataclasses

import numpy as np

A_HUBER, LAMBDA_0, FTOL, PTOL, DECREASE, INCREASE, MAX_ITERATIONS = 1.5, 1e-4, 1e-10, 1e-10, 2.0, 10.0, 50
MIN_DEPTH, BORDER = 0.001, 4
FUNCTION_TOLERANCE, PARAMETER_TOLERANCE, NO_VALID_RESIDUAL = 1, 2, 4


@dataclasses.dataclass
class Problem:
    cam: tuple
    poses: np.ndarray
    X: np.ndarray
    off: np.ndarray
    ofr: np.ndarray
    oxy: np.ndarray

    def __post_init__(self):
        self.off = np.ascontiguousarray(self.off, np.int32)
        self.ofr = np.ascontiguousarray(self.ofr, np.int32)
        self.oxy = np.ascontiguousarray(self.oxy, np.float64).reshape(-1, 2)
        self.poses = np.ascontiguousarray(self.poses).reshape(-1, 12)
        self.X = np.ascontiguousarray(self.X).reshape(-1, 3)
        self.obl = np.repeat(np.arange(len(self.off) - 1), np.diff(self.off)).astype(np.int64)

    @property
    def F(self):
        return len(self.poses)

    @property
    def L(self):
        return len(self.X)

    @property
    def M(self):
        return len(self.ofr)

    def with_state(self, poses, X):
        return Problem(self.cam, np.array(poses), np.array(X), self.off, self.ofr, self.oxy)


def pose_parts(poses):
    return poses[:, :9].reshape(-1, 3, 3), poses[:, 9:]


def hat(v):
    z = np.zeros_like(v[..., 0])
    return np.stack([np.stack([z, -v[..., 2], v[..., 1]], -1), np.stack([v[..., 2], z, -v[..., 0]], -1),
                     np.stack([-v[..., 1], v[..., 0], z], -1)], -2)


def _series(th2, first, dtype, terms=12):
    """sum_k (-1)^k th2^k / (first + 2 k)!, exact coefficients in dtype"""
    out, fact, power = dtype(0), dtype(1), dtype(1)
    for m in range(2, first + 1):
        fact = fact * dtype(m)
    for k in range(terms):
        out = out + (power / fact if k % 2 == 0 else -power / fact)
        power = power * th2
        fact = fact * dtype(first + 2 * k + 1) * dtype(first + 2 * k + 2)
    return out


def exp_se3(xi, dtype=np.float64):
    """(R, t) of exp(upsilon, omega): R = I + A W + B W^2, t = (I + B W + C W^2) upsilon; the series below |omega|^2 = 0.25"""
    xi = np.asarray(xi, dtype)
    w = xi[3:]
    th2 = w @ w
    if th2 < 0.25:
        A, B, Cc = _series(th2, 1, dtype), _series(th2, 2, dtype), _series(th2, 3, dtype)
    else:
        th = np.sqrt(th2)
        A, B, Cc = np.sin(th) / th, (1 - np.cos(th)) / th2, (th - np.sin(th)) / (th2 * th)
    W = hat(w)
    W2 = np.outer(w, w) - th2 * np.eye(3, dtype=dtype)
    eye = np.eye(3, dtype=dtype)
    return eye + A * W + B * W2, (eye + B * W + Cc * W2) @ xi[:3]


def sphere_basis(d):
    k = int(np.argmin(np.abs(d)))          # the first axis with the smallest |d_k|
    e = np.zeros(3, d.dtype)
    e[k] = 1
    c = np.cross(d, e)
    b1 = c / np.sqrt(c @ c)
    return b1, np.cross(d, b1)


def huber(s, a):
    big = s > a * a
    n = np.sqrt(np.where(big, s, 1))
    return np.where(big, a / n, 1), np.where(big, 2 * a * n - a * a, s)


def project(pr, dtype=np.float64):
    """valid (M,), q (M, 2), pc (M, 3) of every observation; the thresholds' margins (px, depth) for the near-decision rule"""
    fx, fy, cx, cy, width, height = pr.cam
    R, t = pose_parts(pr.poses.astype(dtype))
    X = pr.X.astype(dtype)
    pc = np.einsum("mij,mj->mi", R[pr.ofr], X[pr.obl]) + t[pr.ofr]
    front = pc[:, 2] >= MIN_DEPTH
    z = np.where(front, pc[:, 2], 1)
    q = np.stack([dtype(fx) * pc[:, 0] / z + dtype(cx), dtype(fy) * pc[:, 1] / z + dtype(cy)], -1)
    inside = (q[:, 0] >= BORDER) & (q[:, 0] <= width - 1 - BORDER) & (q[:, 1] >= BORDER) & (q[:, 1] <= height - 1 - BORDER)
    return front & inside, q, pc


def decision_margins(pr):
    """per observation, the distance of its validity decision from flipping: |p_z - 0.001| and, where in front, the distance of q to the
    ROI's edges; float64"""
    fx, fy, cx, cy, width, height = pr.cam
    valid, q, pc = project(pr)
    depth = np.abs(pc[:, 2] - MIN_DEPTH)
    edge = np.minimum.reduce([np.abs(q[:, 0] - BORDER), np.abs(q[:, 0] - (width - 1 - BORDER)), np.abs(q[:, 1] - BORDER),
                              np.abs(q[:, 1] - (height - 1 - BORDER))])
    return depth, np.where(pc[:, 2] >= MIN_DEPTH, edge, np.inf)


def evaluate(pr, a=A_HUBER, dtype=np.float64):
    """dict: valid, r (0 where invalid), w (0 where invalid), cost, nvalid"""
    valid, q, _ = project(pr, dtype)
    r = np.where(valid[:, None], pr.oxy.astype(dtype) - q, 0)
    w, rho = huber(np.sum(r * r, -1), dtype(a))
    w = np.where(valid, w, 0)
    return {"valid": valid, "r": r, "w": w, "cost": dtype(0.5) * np.sum(np.where(valid, rho, 0)), "nvalid": int(valid.sum())}


def jacobians(pr, dtype=np.float64):
    """J_x (M, 2, 3) and J_p (M, 2, 6) of r = obs - q for the right increment, zero where invalid"""
    fx, fy = dtype(pr.cam[0]), dtype(pr.cam[1])
    valid, _, pc = project(pr, dtype)
    R, _ = pose_parts(pr.poses.astype(dtype))
    X = pr.X.astype(dtype)
    z = np.where(valid, pc[:, 2], 1)
    G = np.zeros((pr.M, 2, 3), dtype)
    G[:, 0, 0], G[:, 0, 2] = fx / z, -fx * pc[:, 0] / (z * z)
    G[:, 1, 1], G[:, 1, 2] = fy / z, -fy * pc[:, 1] / (z * z)
    Jx = -np.einsum("mij,mjk->mik", G, R[pr.ofr]) * valid[:, None, None]
    A = np.concatenate([np.broadcast_to(np.eye(3, dtype=dtype), (pr.L, 3, 3)), -hat(X)], -1)       # (L, 3, 6)
    return Jx, np.einsum("mij,mjk->mik", Jx, A[pr.obl])


def landmark_factor(Hll, lam):
    """alive (L,), Linv (L, 3, 3) lower with Linv^T Linv = (H_ll + lam diag H_ll)^-1; a pivot <= 0 or not finite kills the landmark"""
    dtype = Hll.dtype.type
    D = Hll + lam * Hll * np.eye(3, dtype=dtype)
    with np.errstate(all="ignore"):
        def ok(d):
            return (d > 0) & np.isfinite(d)
        a00 = D[:, 0, 0]
        alive = ok(a00)
        l00 = np.sqrt(np.where(alive, a00, 1))
        l10, l20 = D[:, 1, 0] / l00, D[:, 2, 0] / l00
        d1 = D[:, 1, 1] - l10 * l10
        alive = alive & ok(d1)
        l11 = np.sqrt(np.where(alive, d1, 1))
        l21 = (D[:, 2, 1] - l20 * l10) / l11
        d2 = D[:, 2, 2] - l20 * l20 - l21 * l21
        alive = alive & ok(d2)
        l22 = np.sqrt(np.where(alive, d2, 1))
        Li = np.zeros_like(D)
        Li[:, 0, 0], Li[:, 1, 1], Li[:, 2, 2] = 1 / l00, 1 / l11, 1 / l22
        Li[:, 1, 0] = -l10 * Li[:, 0, 0] / l11
        Li[:, 2, 1] = -l21 * Li[:, 1, 1] / l22
        Li[:, 2, 0] = -(l20 * Li[:, 0, 0] + l21 * Li[:, 1, 0]) / l22
    Li[~alive] = 0
    return alive, Li


def frame1_basis(pr, norm1, dtype=np.float64):
    """B (6, 5) of frame 1 and (b1, b2): upsilon = norm1 R^T (alpha b1 + beta b2), omega = omega"""
    R, t = pose_parts(pr.poses.astype(dtype))
    d = t[1] / np.sqrt(t[1] @ t[1])
    b1, b2 = sphere_basis(d)
    B = np.zeros((6, 5), dtype)
    B[:3, 0], B[:3, 1] = dtype(norm1) * (R[1].T @ b1), dtype(norm1) * (R[1].T @ b2)
    B[3:, 2:] = np.eye(3, dtype=dtype)
    return B, b1, b2


def free_basis(pr, norm1, dtype=np.float64):
    """(6 (F - 1), n): the six components of frames 1 .. F - 1 from the reduced unknowns, n = 6 (F - 1) - 1"""
    F = pr.F
    n = 6 * (F - 1) - 1
    Bf = np.zeros((6 * (F - 1), n), dtype)
    Bf[:6, :5] = frame1_basis(pr, norm1, dtype)[0]
    Bf[6:, 5:] = np.eye(6 * (F - 2), dtype=dtype)
    return Bf


def linearise(pr, a=A_HUBER, dtype=np.float64):
    """everything of a linearisation that does not depend on lambda"""
    ev = evaluate(pr, a, dtype)
    Jx, Jp = jacobians(pr, dtype)
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
    W = np.einsum("m,mki,mkj->mij", w, Jp, Jx)                                   # (M, 6, 3)
    return dict(ev, Jx=Jx, Jp=Jp, C=C, c=c, Hll=Hll, bl=bl, Hpp=Hpp, bp=bp, W=W)


def reduced_system(pr, lin, lam, norm1, dtype=np.float64):
    """(H (n, n) damped, g (n,), extras) of the statement's reduced system"""
    F, L = pr.F, pr.L
    lam = dtype(lam)
    alive, Li = landmark_factor(lin["Hll"], lam)
    Y = np.einsum("mij,mkj->mik", Li[pr.obl], lin["W"])                           # L^-1 W^T, (M, 3, 6); zero for a dead landmark
    Ybig = np.zeros((L, 3, 6 * F), dtype)
    for k in range(6):
        Ybig[pr.obl, :, 6 * pr.ofr + k] = Y[:, :, k]
    flat = Ybig.reshape(3 * L, 6 * F)
    S = flat.T @ flat
    z = np.einsum("lij,lj->li", Li, lin["bl"])
    rs = flat.T @ z.reshape(3 * L)
    Hbd = np.zeros((6 * F, 6 * F), dtype)
    for f in range(F):
        Hbd[6 * f:6 * f + 6, 6 * f:6 * f + 6] = lin["Hpp"][f]
    Bf = free_basis(pr, norm1, dtype)
    Hm = Bf.T @ Hbd[6:, 6:] @ Bf
    Sm = Bf.T @ S[6:, 6:] @ Bf
    H = Hm - Sm + lam * np.diag(np.diag(Hm))
    g = -(Bf.T @ (lin["bp"].reshape(-1)[6:] - rs[6:]))
    return H, g, dict(alive=alive, Li=Li, Bf=Bf, Hm=Hm, Sm=Sm, S=S, rs=rs)


def cholesky_solve(H, g):
    """x of H x = g by an unblocked Cholesky in H's dtype; None when a pivot is <= 0 or not finite"""
    n = len(g)
    Lm = np.tril(H).copy()
    for k in range(n):
        d = Lm[k, k]
        if not (d > 0 and np.isfinite(d)):
            return None
        Lm[k, k] = np.sqrt(d)
        Lm[k + 1:, k] /= Lm[k, k]
        Lm[k + 1:, k + 1:] -= np.tril(np.outer(Lm[k + 1:, k], Lm[k + 1:, k]))
    y = np.array(g, copy=True)
    for k in range(n):
        y[k] /= Lm[k, k]
        y[k + 1:] -= Lm[k + 1:, k] * y[k]
    for k in range(n - 1, -1, -1):
        y[k] /= Lm[k, k]
        y[:k] -= Lm[k, :k] * y[k]
    return y


def apply_step(pr, lin, lam, norm1, x, a=A_HUBER, dtype=np.float64):
    """the rest of an iteration for the pose step x (reduced coordinates): back-substitution, retraction, the candidate and its cost"""
    F = pr.F
    x = np.asarray(x, dtype)
    lam = dtype(lam)
    B, b1, b2 = frame1_basis(pr, norm1, dtype)
    d6 = np.zeros((F, 6), dtype)
    d6[1] = B @ x[:5]
    d6[2:] = x[5:].reshape(F - 2, 6)
    alive, Li = landmark_factor(lin["Hll"], lam)
    X = pr.X.astype(dtype)
    u = d6[pr.ofr, :3] + np.cross(d6[pr.ofr, 3:], X[pr.obl])
    v = lin["bl"].copy()
    np.add.at(v, pr.obl, np.einsum("mij,mj->mi", lin["C"], u))
    y = np.einsum("lij,lj->li", Li, v)
    dl = -np.einsum("lji,lj->li", Li, y)
    R, t = pose_parts(pr.poses.astype(dtype))
    cand = pr.poses.astype(dtype).copy()
    E1, _ = exp_se3(np.concatenate([np.zeros(3, dtype), d6[1, 3:]]), dtype)
    cand[1, :9] = (R[1] @ E1).reshape(9)
    vdir = t[1] / np.sqrt(t[1] @ t[1]) + x[0] * b1 + x[1] * b2
    cand[1, 9:] = dtype(norm1) * (vdir / np.sqrt(vdir @ vdir))
    for f in range(2, F):
        E, et = exp_se3(d6[f], dtype)
        cand[f, :9] = (R[f] @ E).reshape(9)
        cand[f, 9:] = R[f] @ et + t[f]
    candidate = pr.with_state(cand, X + dl)
    ev = evaluate(candidate, a, dtype)
    step = x @ x + np.sum(dl * dl)
    state = np.sum(t[1:] * t[1:]) + (F - 1) + np.sum(X * X)
    return dict(candidate=candidate, cost=ev["cost"], nvalid=ev["nvalid"], step_sq=step, state_sq=state, dl=dl, d6=d6)


def solve(pr, a=A_HUBER, lambda_0=LAMBDA_0, ftol=FTOL, ptol=PTOL, decrease=DECREASE, increase=INCREASE, max_iterations=MAX_ITERATIONS,
          dtype=np.float64, keep_states=False):
    """the LM driver.  Returns a dict: problem (the final state), initial_cost, final_cost, nvalid, iterations, accepted, converged,
    reason, lambda, trace [(cost_before, cost_candidate, accepted, lambda)], states [(Problem, lambda) each iteration started from]"""
    pr = pr.with_state(pr.poses.astype(dtype), pr.X.astype(dtype))
    t1 = pr.poses[1, 9:]
    norm1 = np.sqrt(t1 @ t1)
    lam = dtype(lambda_0)
    ev = evaluate(pr, a, dtype)
    E, nvalid = ev["cost"], ev["nvalid"]
    out = dict(initial_cost=E, iterations=0, accepted=0, reason=0, trace=[], states=[])
    lin, it = None, 0
    if nvalid == 0:
        out["reason"] = NO_VALID_RESIDUAL
    while it < max_iterations and out["reason"] == 0:
        if lin is None:
            lin = linearise(pr, a, dtype)
        if keep_states:
            out["states"].append((pr, lam))
        H, g, _ = reduced_system(pr, lin, lam, norm1, dtype)
        x = cholesky_solve(H, g)
        it += 1
        if x is None:
            out["trace"].append((E, dtype(np.inf), 0, lam))
            lam = lam * dtype(increase)
            continue
        st = apply_step(pr, lin, lam, norm1, x, a, dtype)
        En = st["cost"]
        if st["nvalid"] == 0:
            out["trace"].append((E, En, 0, lam))
            out["reason"] = NO_VALID_RESIDUAL
            break
        reason = FUNCTION_TOLERANCE if abs(E - En) / E < ftol else 0
        if En < E:
            out["trace"].append((E, En, 1, lam))
            if st["step_sq"] < dtype(ptol) * (st["state_sq"] + dtype(ptol)):
                reason |= PARAMETER_TOLERANCE
            pr, E, nvalid, lin = st["candidate"], En, st["nvalid"], None
            lam = lam / dtype(decrease)
            out["accepted"] += 1
        else:
            out["trace"].append((E, En, 0, lam))
            lam = lam * dtype(increase)
        out["reason"] = reason
    out.update(problem=pr, final_cost=E, nvalid=nvalid, iterations=it, converged=bool(out["reason"] & 3), **{"lambda": lam})
    return out


# ---- triangulation and pruning

def triangulation_matrices(pr):
    """A (L, 4, 4) = sum_i A_i^T A_i over every landmark's observations"""
    fx, fy, cx, cy = pr.cam[:4]
    R, t = pose_parts(pr.poses.astype(np.float64))
    P = np.concatenate([R, t[:, :, None]], -1)[pr.ofr]                            # (M, 3, 4)
    v = np.stack([(pr.oxy[:, 0] - cx) / fx, (pr.oxy[:, 1] - cy) / fy, np.ones(pr.M)], -1)
    v = v / np.sqrt(np.sum(v * v, -1))[:, None]
    Ai = P - v[:, :, None] * np.einsum("mi,mij->mj", v, P)[:, None, :]
    A = np.zeros((pr.L, 4, 4))
    np.add.at(A, pr.obl, np.einsum("mki,mkj->mij", Ai, Ai))
    return A


def triangulate(pr, has_position, min_number_of_projections=4, retriangulation=False):
    """(triangulated (L,) bool, X (L, 3) with the untouched rows as given, eigenvalues (L, 4) ascending)"""
    count = np.diff(pr.off)
    run = (np.asarray(has_position) == 0) | bool(retriangulation)
    run = run & (count > min_number_of_projections)
    vals, vecs = np.linalg.eigh(triangulation_matrices(pr))
    e = vecs[:, :, 0]
    X = np.array(pr.X, np.float64)
    with np.errstate(all="ignore"):
        X[run] = (e[:, :3] / e[:, 3:4])[run]
    return run, X, vals


def flag_outliers(pr, threshold=0.5):
    """flags (M,) bool: not valid, or |obs - q| > threshold"""
    valid, q, _ = project(pr)
    d = pr.oxy - q
    return ~valid | (np.sqrt(np.sum(d * d, -1)) > threshold)


# ---- synthetic scenes shared by the CPU and the GPU tests

def rotation(w):
    return exp_se3(np.concatenate([np.zeros(3), np.asarray(w, float)]))[0]


def make_scene(F=5, L=60, seed=0, cam=(320.0, 310.0, 319.5, 239.5, 640, 480), noise=0.0, outliers=0.0, min_obs=2, max_obs=None,
               depth=(4.0, 9.0)):
    """A camera moving sideways past a cloud of points.  Returns (truth Problem with the noisy observations, rng).  Every landmark is seen
    in between min_obs and max_obs (default F) frames, all of them inside the image with 12 px to spare."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy, width, height = cam
    poses = np.zeros((F, 12))
    for f in range(F):
        Rf = rotation(0.02 * rng.standard_normal(3) * (f > 0))
        c = np.array([0.35 * f, 0.05 * np.sin(f), 0.08 * f]) + 0.02 * rng.standard_normal(3) * (f > 0)   # camera centre in the world
        poses[f, :9], poses[f, 9:] = Rf.reshape(9), -Rf @ c
    R, t = pose_parts(poses)
    X, off, ofr, oxy = [], [0], [], []
    max_obs = F if max_obs is None else min(max_obs, F)
    while len(X) < L:
        z = rng.uniform(*depth)
        mid = 0.175 * (F - 1)
        p = np.array([mid + rng.uniform(-0.55, 0.55) * z, rng.uniform(-0.45, 0.45) * z, z])
        pc = np.einsum("fij,j->fi", R, p) + t
        q = np.stack([fx * pc[:, 0] / pc[:, 2] + cx, fy * pc[:, 1] / pc[:, 2] + cy], -1)
        seen = np.flatnonzero((pc[:, 2] > 1.0) & (q[:, 0] > 16) & (q[:, 0] < width - 17) & (q[:, 1] > 16) & (q[:, 1] < height - 17))
        k = int(rng.integers(min_obs, max_obs + 1))
        if len(seen) < k:
            continue
        frames = np.sort(rng.choice(seen, k, replace=False))
        X.append(p)
        for f in frames:
            o = q[f] + noise * rng.standard_normal(2)
            if rng.uniform() < outliers:
                o = o + rng.uniform(5, 30) * np.array([np.cos(a := rng.uniform(0, 2 * np.pi)), np.sin(a)])
            ofr.append(f)
            oxy.append(o)
        off.append(len(ofr))
    return Problem(cam, poses, np.array(X), np.array(off), np.array(ofr), np.array(oxy)), rng


def perturb(pr, rng, pose_sigma=0.01, point_sigma=0.05):
    """the scene's state moved off the truth: frames >= 1 by a right increment (frame 1 keeps |t_1|), the points by noise"""
    poses = pr.poses.copy()
    R, t = pose_parts(pr.poses)
    for f in range(1, pr.F):
        E, et = exp_se3(pose_sigma * rng.standard_normal(6))
        poses[f, :9] = (R[f] @ E).reshape(9)
        tn = R[f] @ et + t[f]
        if f == 1:
            tn = tn * np.sqrt(t[1] @ t[1]) / np.sqrt(tn @ tn)
        poses[f, 9:] = tn
    return pr.with_state(poses, pr.X + point_sigma * rng.standard_normal(pr.X.shape))


# ---- the bootstrap's track and the three steps of a bootstrap frame (HipRefineTrack of dsopp_amd/host/dsopp_hip_solvers.hpp)

def invert_pose(T):
    """the inverse of 12 doubles (R row-major, t), in the host mirror's order of operations"""
    out = np.zeros(12)
    for r in range(3):
        for c in range(3):
            out[3 * r + c] = T[3 * c + r]
        out[9 + r] = -(T[r] * T[9] + T[3 + r] * T[10] + T[6 + r] * T[11])
    return out


def make_track(F=6, L=150, seed=70, uninitialized=(2,)):
    """(cam, frames, landmarks): frames = dicts frame_id, t_world_agent (12,), initialized; landmarks = dicts has, X (3,), proj = list of
    (frame_id, xy).  Frame ids are not the frames' indices; half of the landmarks carry a (perturbed) position, the others await
    triangulation; the poses are off the truth as a PnP estimate would be."""
    truth, rng = make_scene(F=F, L=L, seed=seed, noise=0.3)
    start = perturb(truth, rng, pose_sigma=0.004, point_sigma=0.03)
    frames = [dict(frame_id=10 + 3 * f, t_world_agent=invert_pose(start.poses[f]), initialized=f not in uninitialized) for f in range(F)]
    landmarks = []
    for l in range(L):
        obs = range(truth.off[l], truth.off[l + 1])
        landmarks.append(dict(has=bool(rng.uniform() < 0.5), X=start.X[l].copy(),
                              proj=[(frames[truth.ofr[o]]["frame_id"], truth.oxy[o].copy()) for o in obs]))
    return truth.cam, frames, landmarks


def _gather(cam, frames, landmarks, local, chosen):
    poses = np.array([invert_pose(frames[i]["t_world_agent"]) for i in local]).reshape(-1, 12)
    X, off, ofr, oxy = [], [0], [], []
    for l in chosen:
        lm = landmarks[l]
        X.append(lm["X"] if lm["has"] else np.zeros(3))
        proj = dict(lm["proj"])
        for f, i in enumerate(local):
            if frames[i]["frame_id"] in proj:
                ofr.append(f)
                oxy.append(proj[frames[i]["frame_id"]])
        off.append(len(ofr))
    return Problem(cam, poses, np.array(X).reshape(-1, 3), np.array(off), np.array(ofr, np.int32), np.array(oxy).reshape(-1, 2))


class ModelBackend:
    """the three calls of a bootstrap frame on the model, the solve in `dtype`; tests/test_gpu_geometric_ba.py has the device's"""

    def __init__(self, dtype=np.float64):
        self.dtype = dtype

    def triangulate(self, pr, has, min_projections, retriangulation):
        run, X, _ = triangulate(pr, has, min_projections, retriangulation)
        return run, X

    def solve(self, pr, a):
        out = solve(pr, a=a, dtype=self.dtype)
        info = dict(iterations=out["iterations"], accepted=out["accepted"], reason=out["reason"], valid=out["nvalid"],
                    initial_cost=float(out["initial_cost"]), final_cost=float(out["final_cost"]))
        return out["problem"].poses.astype(np.float64), out["problem"].X.astype(np.float64), info

    def flag_outliers(self, pr, threshold):
        return flag_outliers(pr, threshold)


def bootstrap_frame(backend, cam, frames, landmarks, min_projections=4, window=10, a=A_HUBER, outlier_threshold=0.5):
    """triangulatePoints, optimizeTransformations, removeOutliers over `frames` (the frames so far), in place; returns the step's record"""
    everything = list(range(len(landmarks)))
    pr = _gather(cam, frames, landmarks, list(range(len(frames))), everything)
    done, X = backend.triangulate(pr, np.array([lm["has"] for lm in landmarks], np.uint8), min_projections, False)
    for l in np.flatnonzero(done):
        landmarks[l]["has"], landmarks[l]["X"] = True, np.array(X[l])
    start = len(frames) - min(len(frames), window)
    ids = [frames[i]["frame_id"] for i in range(start, len(frames))]
    chosen = [l for l, lm in enumerate(landmarks) if lm["has"] and any(fid in ids for fid, _ in lm["proj"])]
    local = [i for i in range(start, len(frames)) if frames[i]["initialized"]]
    info = dict(iterations=0, accepted=0, reason=0, valid=0, initial_cost=0.0, final_cost=0.0)
    if len(local) >= 2:
        pr = _gather(cam, frames, landmarks, local, chosen)
        poses, X, info = backend.solve(pr, a)
        for f, i in enumerate(local):
            frames[i]["t_world_agent"] = invert_pose(np.asarray(poses[f], np.float64))
        for k, l in enumerate(chosen):
            landmarks[l]["X"] = np.array(X[k], np.float64)
    removed = 0
    chosen = [l for l, lm in enumerate(landmarks) if lm["has"]]
    if local:
        pr = _gather(cam, frames, landmarks, local, chosen)
        flags = np.asarray(backend.flag_outliers(pr, outlier_threshold)).astype(bool)
        for k, l in enumerate(chosen):
            gone = {frames[local[pr.ofr[o]]]["frame_id"] for o in range(pr.off[k], pr.off[k + 1]) if flags[o]}
            landmarks[l]["proj"] = [(fid, xy) for fid, xy in landmarks[l]["proj"] if fid not in gone]
        removed = int(flags.sum())
    return dict(info, triangulated=int(np.sum(done)), removed=removed)


def run_bootstrap(backend, track, steps=3):
    """the last `steps` frames arrive one by one; returns (frames, landmarks, records) of a deep copy of the track"""
    import copy
    cam, frames, landmarks = copy.deepcopy(track)
    records = []
    for step in range(steps):
        records.append(bootstrap_frame(backend, cam, frames[:len(frames) - steps + step + 1], landmarks))
    return frames, landmarks, records


def write_track_file(path, track, steps, width=None, height=None):
    """the input of dsopp_amd/host/example_refine_track.cpp"""
    import struct
    cam, frames, landmarks = track
    with open(path, "wb") as f:
        f.write(f"{width or cam[4]} {height or cam[5]} {len(frames)} {len(landmarks)} {steps}\n".encode())
        f.write(struct.pack("<4d", *cam[:4]))
        for fr in frames:
            f.write(struct.pack("<2i12d", fr["frame_id"], int(fr["initialized"]), *fr["t_world_agent"]))
        for lm in landmarks:
            f.write(struct.pack("<2i3d", int(lm["has"]), len(lm["proj"]), *lm["X"]))
            for fid, xy in lm["proj"]:
                f.write(struct.pack("<i2d", fid, *xy))
