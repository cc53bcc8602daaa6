"""The NumPy statement of the bootstrap's PnP RANSAC (include/dsopp_hip.h, dsopp_hip_pnp_ransac_estimate): the three-point pose by
Grunert's elimination with numpy.roots, the angular inlier test, the selection, the LM refinement over the winner's inliers, the final
selection, and initializePoses' decision over the returned pair.  Written from the header's text, not from the kernel.  Everything is
binary64.  tests/test_pnp_ransac.py pins it on the CPU, tests/test_gpu_pnp_ransac.py holds the device to it.

A pose is (R, t), world to camera: p = R X + t.  As 12 doubles it is R row-major, then t (the geometric BA's t_agent_world layout)."""
from collections import namedtuple

import numpy as np

import geometric_ba_model as gm
from rotation_ransac_model import Camera, roi, unproject

Solution = namedtuple("Solution", "R t u v s1")
Hypotheses = namedtuple("Hypotheses", "num_solutions poses counts distances")
Refinement = namedtuple("Refinement", "pose iterations flags cost_initial cost_final trace")
Result = namedtuple("Result", "matches best_iteration best_solution ransac_inlier_count pose_ransac ransac_inliers refined_inlier_count "
                              "refine_iterations refine_flags cost_initial cost_final pose inliers distances trace")

LAMBDA_0, FTOL, PTOL, DECREASE, INCREASE, MAX_ITERATIONS = 1e-4, 1e-10, 1e-10, 2.0, 10.0, 10
MIN_DEPTH = 0.001
FUNCTION_TOLERANCE, PARAMETER_TOLERANCE, NO_VALID_RESIDUAL = 1, 2, 4
DEFAULT_ITERATIONS = 256
IDENTITY = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])


def angular_threshold(cam, threshold_px=0.5):
    """estimate_se3_pnp.cpp:45"""
    return 1.0 - np.cos(np.arctan(np.float64(threshold_px) / np.float64(cam.fx)))


def bearings(cam, obs):
    """f_j = normalize(unproject(obs[j])), per row"""
    u = unproject(cam, obs)
    return u / np.sqrt(u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1] + u[:, 2] * u[:, 2])[:, None]


def pose12(R, t):
    return np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)])


def pose_parts(pose):
    pose = np.asarray(pose, np.float64)
    return pose[:9].reshape(3, 3), pose[9:]


# ---- the three-point pose

def triangle_is_degenerate(X):
    d12, d13 = X[1] - X[0], X[2] - X[0]
    c = np.cross(d12, d13)
    return bool(d13 @ d13 == 0.0 or not c @ c > 1e-12 * (d12 @ d12) * (d13 @ d13))


def quartic(X, f):
    """(c4 .. c0 of the quartic in v, and what u(v) and s1(v) need) for world points X (3, 3) and unit bearings f (3, 3)"""
    a2, b2, c2 = (X[1] - X[2]) @ (X[1] - X[2]), (X[0] - X[2]) @ (X[0] - X[2]), (X[0] - X[1]) @ (X[0] - X[1])
    ca, cb, cg = f[1] @ f[2], f[0] @ f[2], f[0] @ f[1]
    K, m = (a2 - c2) / b2, c2 / b2
    n2, n1, n0 = K - 1.0, -2.0 * K * cb, 1.0 + K
    d1, d0 = -2.0 * ca, 2.0 * cg
    q1 = -2.0 * cb
    c4 = n2 * n2 - m * d1 * d1
    c3 = 2.0 * n2 * n1 - 2.0 * cg * n2 * d1 - m * (2.0 * d0 * d1 + q1 * d1 * d1)
    c2_ = d1 * d1 + n1 * n1 + 2.0 * n2 * n0 - 2.0 * cg * (n2 * d0 + n1 * d1) - m * (d0 * d0 + 2.0 * q1 * d0 * d1 + d1 * d1)
    c1 = 2.0 * d0 * d1 + 2.0 * n1 * n0 - 2.0 * cg * (n1 * d0 + n0 * d1) - m * (q1 * d0 * d0 + 2.0 * d0 * d1)
    c0 = d0 * d0 + n0 * n0 - 2.0 * cg * n0 * d0 - m * d0 * d0
    return np.array([c4, c3, c2_, c1, c0]), dict(N=(n2, n1, n0), D=(d1, d0), q1=q1, b2=b2)


def real_roots(coefficients):
    """the real roots numpy.roots finds (LAPACK returns a real eigenvalue with a zero imaginary part), each polished by two Newton steps"""
    if not np.all(np.isfinite(coefficients)):
        return np.zeros(0)
    z = np.roots(coefficients)
    v = np.sort(z.real[z.imag == 0.0])
    p, dp = np.poly1d(coefficients), np.poly1d(coefficients).deriv()
    for _ in range(2):
        with np.errstate(all="ignore"):
            step = p(v) / dp(v)
        v = np.where(np.isfinite(step), v - step, v)
    return np.sort(v)


def frame(P):
    """[e1 e2 e3] of a triangle's three points (rows of P)"""
    d = P[1] - P[0]
    e1 = d / np.sqrt(d @ d)
    c = np.cross(e1, P[2] - P[0])
    e3 = c / np.sqrt(c @ c)
    return np.stack([e1, np.cross(e3, e1), e3], axis=1)


def p3p(X, f):
    """the solutions of one triple in ascending v; X (3, 3) world points, f (3, 3) unit bearings.  No roi test here"""
    X, f = np.asarray(X, np.float64), np.asarray(f, np.float64)
    if triangle_is_degenerate(X):
        return []
    coefficients, aux = quartic(X, f)
    out = []
    for v in real_roots(coefficients):
        n2, n1, n0 = aux["N"]
        d1, d0 = aux["D"]
        with np.errstate(all="ignore"):
            u = ((n2 * v + n1) * v + n0) / (d1 * v + d0)
            Q = (v + aux["q1"]) * v + 1.0
        if not (v > 0.0 and u > 0.0 and Q > 0.0):
            continue
        s1 = np.sqrt(aux["b2"] / Q)
        Y = np.stack([s1 * f[0], (u * s1) * f[1], (v * s1) * f[2]])
        R = frame(Y) @ frame(X).T
        t = Y[0] - R @ X[0]
        if np.all(np.isfinite(R)) and np.all(np.isfinite(t)):
            out.append(Solution(R, t, u, v, s1))
    return out[:4]


# ---- score and selection

def distances(R, t, X, f, ok):
    """d_j = 1 - f_j . p / |p| with p = R X_j + t; NaN for a non-match (never an inlier)"""
    X = np.asarray(X, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        p = np.stack([R[k, 0] * X[:, 0] + R[k, 1] * X[:, 1] + R[k, 2] * X[:, 2] + t[k] for k in range(3)], axis=1)
        norm = np.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1] + p[:, 2] * p[:, 2])
        d = 1.0 - (f[:, 0] * p[:, 0] + f[:, 1] * p[:, 1] + f[:, 2] * p[:, 2]) / norm
    return np.where(ok, d, np.nan)


def inlier_mask(d, t_ang):
    with np.errstate(invalid="ignore"):
        return d < t_ang  # (strict; False for a NaN)


def hypotheses(cam, X, obs, samples, t_ang):
    """every solution of every hypothesis scored against all points; unused solution slots hold zero poses, zero counts, NaN distances"""
    X, obs = np.asarray(X, np.float64).reshape(-1, 3), np.asarray(obs, np.float64).reshape(-1, 2)
    samples = np.asarray(samples, np.int64).reshape(-1, 3)
    ok, f = roi(cam, obs), bearings(cam, obs)
    m, n = len(samples), len(X)
    num, poses, counts = np.zeros(m, np.int64), np.zeros((m, 4, 12)), np.zeros((m, 4), np.int64)
    dist = np.full((m, 4, n), np.nan)
    for i, s in enumerate(samples):
        if not ok[s].all():
            continue
        for k, sol in enumerate(p3p(X[s], f[s])):
            poses[i, k] = pose12(sol.R, sol.t)
            dist[i, k] = distances(sol.R, sol.t, X, f, ok)
            counts[i, k] = inlier_mask(dist[i, k], t_ang).sum()
            num[i] = k + 1
    return Hypotheses(num, poses, counts, dist)


def select(counts):
    """(best_iteration, best_solution, count): the greatest count, the lowest hypothesis, then the lowest solution; -1 when none exceeds 0"""
    counts = np.asarray(counts).reshape(-1, 4)
    if counts.size == 0 or counts.max() <= 0:
        return -1, -1, 0
    best = counts.max(axis=1)
    i = int(np.argmax(best))
    return i, int(np.argmax(counts[i])), int(best[i])


# ---- the refinement

def residuals(cam, pose, X, obs):
    """(counts (k,), r (k, 2) zero where not counted, p (k, 3)) of the pixel residual obs - q"""
    R, t = pose_parts(pose)
    p = np.stack([R[k, 0] * X[:, 0] + R[k, 1] * X[:, 1] + R[k, 2] * X[:, 2] + t[k] for k in range(3)], axis=1)
    front = p[:, 2] >= MIN_DEPTH
    z = np.where(front, p[:, 2], 1.0)
    q = np.stack([cam.fx * p[:, 0] / z + cam.cx, cam.fy * p[:, 1] / z + cam.cy], axis=1)
    return front, np.where(front[:, None], obs - q, 0.0), p


def cost(cam, pose, X, obs):
    front, r, _ = residuals(cam, pose, X, obs)
    return 0.5 * np.sum(r * r), int(front.sum())


def linearise(cam, pose, X, obs):
    """(H (6, 6), b (6,)) = sum J^T J, sum J^T r with J = -G R [I | -hat(X)] for the right increment T <- T exp(delta)"""
    R, _ = pose_parts(pose)
    front, r, p = residuals(cam, pose, X, obs)
    z = np.where(front, p[:, 2], 1.0)
    G = np.zeros((len(X), 2, 3))
    G[:, 0, 0], G[:, 0, 2] = cam.fx / z, -cam.fx * p[:, 0] / (z * z)
    G[:, 1, 1], G[:, 1, 2] = cam.fy / z, -cam.fy * p[:, 1] / (z * z)
    A = np.concatenate([np.broadcast_to(np.eye(3), (len(X), 3, 3)), -gm.hat(X)], axis=-1)
    J = -np.einsum("kij,jl,klm->kim", G, R, A) * front[:, None, None]
    return np.einsum("kij,kil->jl", J, J), np.einsum("kij,ki->j", J, r)


def retract(pose, delta):
    R, t = pose_parts(pose)
    E, et = gm.exp_se3(delta)
    return pose12(R @ E, R @ et + t)


def refine(cam, pose, X, obs, lambda_0=LAMBDA_0, ftol=FTOL, ptol=PTOL, decrease=DECREASE, increase=INCREASE, max_iterations=MAX_ITERATIONS):
    """the geometric BA's LM driver over one pose with the landmarks fixed.  trace: per iteration (cost_before, cost_candidate, accepted,
    lambda, |dE| / E / ftol, |delta|^2 / (ptol (state + ptol)))"""
    X, obs = np.asarray(X, np.float64).reshape(-1, 3), np.asarray(obs, np.float64).reshape(-1, 2)
    pose = np.array(pose, np.float64)
    lam = np.float64(lambda_0)
    E, nvalid = cost(cam, pose, X, obs)
    E0, flags, it, lin, trace = E, 0, 0, None, []
    if nvalid == 0:
        flags = NO_VALID_RESIDUAL
    while it < max_iterations and flags == 0:
        if lin is None:
            lin = linearise(cam, pose, X, obs)
        H, b = lin
        delta = gm.cholesky_solve(H + lam * np.diag(np.diag(H)), -b)
        it += 1
        if delta is None:
            trace.append((E, np.inf, 0, lam, np.inf, np.inf))
            lam = lam * increase
            continue
        cand = retract(pose, delta)
        En, nv = cost(cam, cand, X, obs)
        with np.errstate(all="ignore"):
            rf = np.float64(abs(E - En)) / E
            rp = (delta @ delta) / (ptol * (pose[9:] @ pose[9:] + 1.0 + ptol))
        if nv == 0:
            trace.append((E, En, 0, lam, rf / ftol, rp))
            flags = NO_VALID_RESIDUAL
            break
        reason = FUNCTION_TOLERANCE if rf < ftol else 0
        accepted = bool(En < E)
        trace.append((E, En, int(accepted), lam, rf / ftol, rp))
        if accepted:
            if delta @ delta < ptol * (pose[9:] @ pose[9:] + 1.0 + ptol):
                reason |= PARAMETER_TOLERANCE
            pose, E, lin = cand, En, None
            lam = lam / decrease
        else:
            lam = lam * increase
        flags = reason
    return Refinement(pose, it, flags, E0, E, trace)


# ---- the whole call

def estimate(cam, X, obs, samples, threshold_px=0.5, max_iterations=MAX_ITERATIONS, hyp=None):
    """(Result, Hypotheses) of dsopp_hip_pnp_ransac_estimate; `hyp`: the hypotheses when they are known already"""
    X, obs = np.asarray(X, np.float64).reshape(-1, 3), np.asarray(obs, np.float64).reshape(-1, 2)
    t_ang = angular_threshold(cam, threshold_px)
    ok = roi(cam, obs)
    f = bearings(cam, obs)
    h = hyp if hyp is not None else hypotheses(cam, X, obs, samples, t_ang)
    i, k, count = select(h.counts)
    none = np.zeros(0, np.int64)
    if i < 0:
        return Result(int(ok.sum()), -1, -1, 0, IDENTITY.copy(), none, 0, 0, 0, 0.0, 0.0, IDENTITY.copy(), none, np.full(len(X), np.nan), []), h
    pose_ransac = h.poses[i, k]
    ransac_inliers = np.flatnonzero(inlier_mask(h.distances[i, k], t_ang))
    ref = refine(cam, pose_ransac, X[ransac_inliers], obs[ransac_inliers], max_iterations=max_iterations)
    d = distances(*pose_parts(ref.pose), X, f, ok)
    inliers = np.flatnonzero(inlier_mask(d, t_ang))
    return Result(int(ok.sum()), i, k, count, pose_ransac, ransac_inliers, len(inliers), ref.iterations, ref.flags, ref.cost_initial,
                  ref.cost_final, ref.pose, inliers, d, ref.trace), h


def initialised(inliers, matches, ratio=0.5):
    """initializePoses' rule (initialize_poses.cpp:47-73): inliers > (size_t)(ratio * matches), with the truncation"""
    return bool(inliers > int(np.float64(ratio) * np.float64(matches)))


# ---- the synthetic scene shared by the CPU and the GPU tests

CAM = Camera(448.0, 448.0, 320.0, 240.0, 640, 480)
TRUE_POSE = pose12(gm.exp_se3([0, 0, 0, 0.03, -0.05, 0.02])[0], [0.2, -0.1, 0.3])


def make_scene(n, seed, noise=0.3, outliers=0.3, outlier_sigma=15.0, cam=CAM, pose=TRUE_POSE, depth=(2.0, 10.0)):
    """n points at `depth` metres in front of the camera at `pose`, seen inside the ROI; the observations carry N(0, noise) px, and a share
    `outliers` of them is displaced by N(0, outlier_sigma) px (and kept inside the ROI by redrawing).  Returns (X, obs)"""
    rng = np.random.default_rng(seed)
    R, t = pose_parts(pose)
    px = np.stack([rng.uniform(8.0, cam.width - 9.0, n), rng.uniform(8.0, cam.height - 9.0, n)], axis=1)
    pc = unproject(cam, px) * rng.uniform(depth[0], depth[1], n)[:, None]
    X = (pc - t) @ R                                   # R^T (p - t), per row
    obs = px + noise * rng.standard_normal((n, 2))
    for j in np.flatnonzero(rng.random(n) < outliers):
        while True:
            o = obs[j] + outlier_sigma * rng.standard_normal(2)
            if roi(cam, o)[0]:
                break
        obs[j] = o
    return X, np.where(roi(cam, obs)[:, None], obs, px)


def draw_triples(rng, n, count):
    return np.array([rng.choice(n, 3, replace=False) for _ in range(count)], np.int32).reshape(-1, 3)
