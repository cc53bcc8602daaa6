"""The NumPy statement of the bootstrap's two-view pose (include/dsopp_hip.h, dsopp_hip_two_view_ransac_*): the five-point essential
matrices of a sample through the action matrix and numpy.linalg.eig, their poses, the two-view angular measure, the selection, the
Sampson refinement run twice around the re-selection, the two-view triangulation, and initializePoses' decision over the returned
pair.  Written from the header's text, not from the kernel.  Everything is binary64.  tests/test_two_view_ransac.py pins it on the CPU,
tests/test_gpu_two_view_ransac.py holds the device to it.

A pose is (R, t) with |t| = 1 and p_A = R p_B + t: it maps the last frame (B) into the first (A).  As 12 doubles it is R row-major, then t."""
import itertools
from collections import namedtuple

import numpy as np

import geometric_ba_model as gm
from pnp_ransac_model import angular_threshold, bearings, inlier_mask, pose12, pose_parts
from rotation_ransac_model import Camera, roi

Hypotheses = namedtuple("Hypotheses", "num_solutions poses counts distances")
Refinement = namedtuple("Refinement", "pose iterations flags cost_initial cost_final trace")
Result = namedtuple("Result", "matches best_iteration best_solution ransac_inlier_count inlier_count stages pose_ransac pose_reselect pose "
                              "ransac_inliers inliers distances")

LAMBDA_0, FTOL, PTOL, DECREASE, INCREASE, MAX_ITERATIONS, A_HUBER = 1e-4, 1e-10, 1e-10, 2.0, 10.0, 40, 1.5
FUNCTION_TOLERANCE, PARAMETER_TOLERANCE, NO_VALID_RESIDUAL = 1, 2, 4
DEFAULT_ITERATIONS, MIN_MATCHES, MAX_SOLUTIONS = 256, 50, 10
COS_THRESHOLD = 0.9999
IDENTITY = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])
POLISH_STEPS = 12
CONSTRAINT_TOLERANCE = 1e-9

# monomials of degree <= 3 in (x, y, z) as sorted triples over (x, y, z, 1) = (0, 1, 2, 3)
X_, Y_, Z_, W_ = 0, 1, 2, 3
CUBICS = [(0, 0, 0), (0, 0, 1), (0, 1, 1), (1, 1, 1), (0, 0, 2), (0, 1, 2), (1, 1, 2), (0, 2, 2), (1, 2, 2), (2, 2, 2)]
LOWER = [(0, 0, 3), (0, 1, 3), (1, 1, 3), (0, 2, 3), (1, 2, 3), (2, 2, 3), (0, 3, 3), (1, 3, 3), (2, 3, 3), (3, 3, 3)]
ACTION_ORDER = CUBICS + LOWER  # the ten cubic monomials, then x^2 xy y^2 xz yz z^2 x y z 1
# the hidden-variable order: x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1
HIDDEN_ORDER = [(0, 0, 0), (1, 1, 1), (0, 0, 1), (0, 1, 1), (0, 0, 2), (0, 0, 3), (1, 1, 2), (1, 1, 3), (0, 1, 2), (0, 1, 3),
                (0, 2, 2), (0, 2, 3), (0, 3, 3), (1, 2, 2), (1, 2, 3), (1, 3, 3), (2, 2, 2), (2, 2, 3), (2, 3, 3), (3, 3, 3)]


# ---- the five-point essential matrices

def null_basis(fa, fb):
    """an orthonormal basis (4, 3, 3) of the E with f_A . E f_B = 0 for the five pairs"""
    Q = np.stack([np.kron(fa[k], fb[k]) for k in range(5)])
    return np.linalg.svd(Q)[2][5:].reshape(4, 3, 3)


HADAMARD = np.array([[1.0, 1.0, 1.0, 1.0], [1.0, -1.0, 1.0, -1.0], [1.0, 1.0, -1.0, -1.0], [1.0, -1.0, -1.0, 1.0]]) / 2.0


def elimination_basis(fa, fb, mix=True):
    """the basis the device builds, for the record (any basis serves): a fully pivoted Gauss-Jordan elimination of the 5 x 9 constraints,
    its four null vectors made orthonormal by Gram-Schmidt, then mixed by a Hadamard matrix.  Without the mix a coordinate ratio in the
    basis is a ratio of two entries of E, which the solutions of a small-motion scene nearly share: the hidden variable of the polynomial
    route then fails to separate them (tests/test_two_view_ransac.py shows the sample that found it)"""
    Q = np.stack([np.kron(fa[k], fb[k]) for k in range(5)])
    perm = list(range(9))
    for k in range(5):
        sub = np.abs(Q[k:, k:])
        at = int(np.argmax(sub))
        pr, pc = k + at // sub.shape[1], k + at % sub.shape[1]
        Q[[k, pr]] = Q[[pr, k]]
        Q[:, [k, pc]] = Q[:, [pc, k]]
        perm[k], perm[pc] = perm[pc], perm[k]
        row = Q[k] / Q[k, k]
        for r in range(5):
            Q[r] = row if r == k else Q[r] - Q[r, k] * row
    nv = np.zeros((4, 9))
    for j in range(4):
        x = np.zeros(9)
        x[:5], x[5 + j] = -Q[:, 5 + j], 1.0
        nv[j, perm] = x
    for j in range(4):
        for _ in range(2):
            for i in range(j):
                nv[j] = nv[j] - (nv[i] @ nv[j]) * nv[i]
        nv[j] = nv[j] / np.sqrt(nv[j] @ nv[j])
    return ((HADAMARD @ nv) if mix else nv).reshape(4, 3, 3)


def trilinear(Ea, Eb, Ec):
    """the ten constraints polarised: det of (row 0 of Ea, row 1 of Eb, row 2 of Ec), then 2 Ea Eb^T Ec - tr(Ea Eb^T) Ec row by row;
    over any leading axes"""
    b, c = Eb[..., 1, :], Ec[..., 2, :]
    d = Ea[..., 0, 0] * (b[..., 1] * c[..., 2] - b[..., 2] * c[..., 1]) + Ea[..., 0, 1] * (b[..., 2] * c[..., 0] - b[..., 0] * c[..., 2]) + \
        Ea[..., 0, 2] * (b[..., 0] * c[..., 1] - b[..., 1] * c[..., 0])
    M = Ea @ np.swapaxes(Eb, -1, -2)
    rest = 2.0 * M @ Ec - np.trace(M, axis1=-2, axis2=-1)[..., None, None] * Ec
    return np.concatenate([d[..., None], rest.reshape(rest.shape[:-2] + (9,))], axis=-1)


def constraints(E):
    return trilinear(E, E, E)


_ABC = np.array(list(itertools.product(range(4), repeat=3)))


def coefficient_matrix(basis, order):
    """the 10 x 20 matrix of the ten cubics in (x, y, z) of E = x E1 + y E2 + z E3 + E4, columns in `order`"""
    col = {m: k for k, m in enumerate(order)}
    T = trilinear(basis[_ABC[:, 0]], basis[_ABC[:, 1]], basis[_ABC[:, 2]])
    A = np.zeros((10, 20))
    for abc, row in zip(_ABC, T):
        A[:, col[tuple(sorted(abc))]] += row
    return A


def essential_of(basis, p):
    return p[0] * basis[0] + p[1] * basis[1] + p[2] * basis[2] + basis[3]


def polish(basis, p, steps=POLISH_STEPS):
    """Gauss-Newton on the ten cubics in the null-space coordinates, until the point stops moving"""
    p = np.array(p, np.float64)
    for _ in range(steps):
        E = essential_of(basis, p)
        r = constraints(E)
        J = (trilinear(basis[:3], E, E) + trilinear(E, basis[:3], E) + trilinear(E, E, basis[:3])).T
        with np.errstate(all="ignore"):
            try:
                step = np.linalg.solve(J.T @ J, -(J.T @ r))
            except np.linalg.LinAlgError:
                break
        if not np.all(np.isfinite(step)):
            break
        p = p + step
        if step @ step <= 1e-28 * (1.0 + p @ p):  # (the next step would be its square)
            break
    return p


def five_point(fa, fb, route="action", basis=None):
    """the real essential matrices (k, 3, 3) of five pairs of unit bearings, each of Frobenius norm sqrt 2.  route "action": the action
    matrix of x on the quotient ring and numpy.linalg.eig; route "hidden": the 10th-degree polynomial in z and numpy.roots.  basis: another
    orthonormal basis of the null space than the SVD's"""
    basis = null_basis(np.asarray(fa, np.float64), np.asarray(fb, np.float64)) if basis is None else basis
    with np.errstate(all="ignore"):
        try:
            points = _action_route(basis) if route == "action" else _hidden_route(basis)
        except np.linalg.LinAlgError:
            return np.zeros((0, 3, 3)), basis
    out = []
    for p in points:
        if not np.all(np.isfinite(p)):
            continue
        E = essential_of(basis, polish(basis, p))
        n2 = np.sum(E * E)
        if np.isfinite(n2) and n2 > 0.0:
            E = E * np.sqrt(2.0 / n2)
            if np.max(np.abs(constraints(E))) <= CONSTRAINT_TOLERANCE:  # (the polish has reached the constraints)
                out.append(E)
    return np.array(out).reshape(-1, 3, 3), basis


def _action_route(basis):
    A = coefficient_matrix(basis, ACTION_ORDER)
    M = np.linalg.solve(A[:, :10], A[:, 10:])  # cubic monomial k = -M[k] . (x^2 xy y^2 xz yz z^2 x y z 1)
    row = {m: k for k, m in enumerate(CUBICS)}
    low = {m: k for k, m in enumerate(LOWER)}
    Ax = np.zeros((10, 10))
    for k, m in enumerate(LOWER):
        prod = tuple(sorted((X_,) + tuple(v for v in m if v != W_) + (W_,) * (m.count(W_) - 1)))
        if prod in row:
            Ax[k] = -M[row[prod]]
        else:
            Ax[k, low[prod]] = 1.0
    w, V = np.linalg.eig(Ax)
    return [(V[6:9, k] / V[9, k]).real for k in range(10) if w[k].imag == 0.0]


def hidden_polynomial(basis):
    """(c (11,) highest power first, the 3 x 3 matrix of polynomials B(z) as B[r][c] highest power first) of the hidden-variable form"""
    A = coefficient_matrix(basis, HIDDEN_ORDER)
    G = np.linalg.solve(A[:, :10], A[:, 10:])
    B = []
    for e, f in ((4, 5), (6, 7), (8, 9)):
        px = np.array([-G[f, 0], G[e, 0] - G[f, 1], G[e, 1] - G[f, 2], G[e, 2]])
        py = np.array([-G[f, 3], G[e, 3] - G[f, 4], G[e, 4] - G[f, 5], G[e, 5]])
        p1 = np.array([-G[f, 6], G[e, 6] - G[f, 7], G[e, 7] - G[f, 8], G[e, 8] - G[f, 9], G[e, 9]])
        B.append((px, py, p1))
    def minor(r0, r1, c0, c1):
        return np.polysub(np.polymul(B[r0][c0], B[r1][c1]), np.polymul(B[r0][c1], B[r1][c0]))
    c = np.polyadd(np.polysub(np.polymul(B[0][0], minor(1, 2, 1, 2)), np.polymul(B[0][1], minor(1, 2, 0, 2))), np.polymul(B[0][2], minor(1, 2, 0, 1)))
    return c, B


def point_of_root(B, z):
    """(x, y, z): (x, y, 1) spans the null space of B(z); from the pair of rows whose cross product has the largest last entry"""
    rows = np.array([[np.polyval(B[r][c], z) for c in range(3)] for r in range(3)])
    best = None
    for r0, r1 in ((0, 1), (0, 2), (1, 2)):
        c = np.cross(rows[r0], rows[r1])
        if best is None or abs(c[2]) > abs(best[2]):
            best = c
    return np.array([best[0] / best[2], best[1] / best[2], z])


def _hidden_route(basis):
    c, B = hidden_polynomial(basis)
    z = np.roots(c)
    return [point_of_root(B, v) for v in np.sort(z.real[z.imag == 0.0])]


# ---- poses

def triangulate_pair(R, t, fa, fb):
    """(alpha, beta, X_A, X_B) per row of the unit bearings fa, fb (triangulation.hpp:29-41)"""
    Rb = np.stack([R[k, 0] * fb[:, 0] + R[k, 1] * fb[:, 1] + R[k, 2] * fb[:, 2] for k in range(3)], axis=1)
    with np.errstate(all="ignore"):
        b = Rb / np.sqrt(Rb[:, 0] * Rb[:, 0] + Rb[:, 1] * Rb[:, 1] + Rb[:, 2] * Rb[:, 2])[:, None]
        ab = fa[:, 0] * b[:, 0] + fa[:, 1] * b[:, 1] + fa[:, 2] * b[:, 2]
        at = fa[:, 0] * t[0] + fa[:, 1] * t[1] + fa[:, 2] * t[2]
        bt = b[:, 0] * t[0] + b[:, 1] * t[1] + b[:, 2] * t[2]
        den = 1.0 / (1.0 - ab * ab)
        alpha, beta = den * (at - ab * bt), den * (ab * at - bt)
        XA = (alpha[:, None] * fa + beta[:, None] * b + t[None, :]) / 2.0
        d = XA - t[None, :]
        XB = np.stack([R[0, k] * d[:, 0] + R[1, k] * d[:, 1] + R[2, k] * d[:, 2] for k in range(3)], axis=1)
    return alpha, beta, XA, XB


def poses_of(E, fa, fb):
    """the pose (R, t) of E under which all five pairs have alpha > 0 and beta > 0, or None"""
    U, _, Vt = np.linalg.svd(E)
    W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    for Wk in (W, W.T):
        R = U @ Wk @ Vt
        if np.linalg.det(R) < 0.0:
            R = -R
        for t in (U[:, 2], -U[:, 2]):
            alpha, beta, _, _ = triangulate_pair(R, t, fa, fb)
            if np.all(alpha > 0.0) and np.all(beta > 0.0) and np.all(np.isfinite(R)) and np.all(np.isfinite(t)):
                return R, t / np.sqrt(t @ t)
    return None


def solve_sample(fa, fb, route="action", basis=None):
    """the poses of a sample (k, 12), k <= 10, in descending trace R"""
    Es, _ = five_point(fa, fb, route, basis)
    found = [p for p in (poses_of(E, fa, fb) for E in Es) if p is not None]
    found.sort(key=lambda p: -np.trace(p[0]))
    return np.array([pose12(R, t) for R, t in found[:MAX_SOLUTIONS]]).reshape(-1, 12)


# ---- measure, score and selection

def distances(R, t, fa, fb, ok):
    """d_j = (1 - f_A . X_A / |X_A|) + (1 - f_B . X_B / |X_B|); NaN for a non-match and for parallel rays (never an inlier)"""
    _, _, XA, XB = triangulate_pair(R, t, fa, fb)
    with np.errstate(all="ignore"):
        na = np.sqrt(XA[:, 0] * XA[:, 0] + XA[:, 1] * XA[:, 1] + XA[:, 2] * XA[:, 2])
        nb = np.sqrt(XB[:, 0] * XB[:, 0] + XB[:, 1] * XB[:, 1] + XB[:, 2] * XB[:, 2])
        d = (1.0 - (fa[:, 0] * XA[:, 0] + fa[:, 1] * XA[:, 1] + fa[:, 2] * XA[:, 2]) / na) + \
            (1.0 - (fb[:, 0] * XB[:, 0] + fb[:, 1] * XB[:, 1] + fb[:, 2] * XB[:, 2]) / nb)
    return np.where(ok, d, np.nan)


def match_mask(cam, A, B):
    return roi(cam, A) & roi(cam, B)


def hypotheses(cam, A, B, samples, t_ang, route="action"):
    A, B = np.asarray(A, np.float64).reshape(-1, 2), np.asarray(B, np.float64).reshape(-1, 2)
    samples = np.asarray(samples, np.int64).reshape(-1, 5)
    ok, fa, fb = match_mask(cam, A, B), bearings(cam, A), bearings(cam, B)
    m, n = len(samples), len(A)
    num, poses, counts = np.zeros(m, np.int64), np.zeros((m, MAX_SOLUTIONS, 12)), np.zeros((m, MAX_SOLUTIONS), np.int64)
    dist = np.full((m, MAX_SOLUTIONS, n), np.nan)
    for i, s in enumerate(samples):
        if not ok[s].all():
            continue
        for k, pose in enumerate(solve_sample(fa[s], fb[s], route)):
            poses[i, k] = pose
            dist[i, k] = distances(*pose_parts(pose), fa, fb, ok)
            counts[i, k] = inlier_mask(dist[i, k], t_ang).sum()
            num[i] = k + 1
    return Hypotheses(num, poses, counts, dist)


def select(counts):
    """(best_iteration, best_solution, count): the greatest count, the lowest hypothesis, then the lowest solution; -1 when none exceeds 0"""
    counts = np.asarray(counts).reshape(-1, MAX_SOLUTIONS)
    if counts.size == 0 or counts.max() <= 0:
        return -1, -1, 0
    best = counts.max(axis=1)
    i = int(np.argmax(best))
    return i, int(np.argmax(counts[i])), int(best[i])


# ---- the refinement

def essential(pose):
    R, t = pose_parts(pose)
    return gm.hat(t) @ R


def _sampson_parts(cam, E, A, B):
    xa = np.stack([(A[:, 0] - cam.cx) / cam.fx, (A[:, 1] - cam.cy) / cam.fx, np.ones(len(A))], axis=1)
    xb = np.stack([(B[:, 0] - cam.cx) / cam.fx, (B[:, 1] - cam.cy) / cam.fx, np.ones(len(B))], axis=1)
    u = np.stack([E[k, 0] * xb[:, 0] + E[k, 1] * xb[:, 1] + E[k, 2] * xb[:, 2] for k in range(3)], axis=1)  # E x_B
    v = np.stack([E[0, k] * xa[:, 0] + E[1, k] * xa[:, 1] + E[2, k] * xa[:, 2] for k in range(3)], axis=1)  # x_A^T E
    top = xa[:, 0] * u[:, 0] + xa[:, 1] * u[:, 1] + xa[:, 2] * u[:, 2]
    bottom = ((u[:, 0] / cam.fx) ** 2 + (u[:, 1] / cam.fx) ** 2) + ((v[:, 0] / cam.fx) ** 2 + (v[:, 1] / cam.fx) ** 2)
    return xa, xb, u, v, top, bottom


def sampson(cam, pose, A, B):
    """r = top / sqrt(bottom) in pixels, top where bottom < 1e-16 (sampson_distance_cost.hpp:17-28)"""
    _, _, _, _, top, bottom = _sampson_parts(cam, essential(pose), A, B)
    small = bottom < 1e-16
    return np.where(small, top, top / np.sqrt(np.where(small, 1.0, bottom)))


def tangent(pose):
    """dE / d(alpha, beta, omega) as (5, 3, 3) at the pose"""
    R, t = pose_parts(pose)
    b1, b2 = gm.sphere_basis(t)
    E = gm.hat(t) @ R
    eye = np.eye(3)
    return np.stack([gm.hat(b1) @ R, gm.hat(b2) @ R] + [E @ gm.hat(eye[k]) for k in range(3)])


def jacobian(cam, pose, A, B):
    """dr / d(alpha, beta, omega), (k, 5), analytic"""
    xa, xb, u, v, top, bottom = _sampson_parts(cam, essential(pose), A, B)
    small = bottom < 1e-16
    safe = np.where(small, 1.0, bottom)
    J = np.zeros((len(A), 5))
    for k, dE in enumerate(tangent(pose)):
        du = xb @ dE.T
        dv = xa @ dE
        dtop = np.sum(xa * du, axis=1)
        dbottom = 2.0 * (u[:, 0] * du[:, 0] + u[:, 1] * du[:, 1] + v[:, 0] * dv[:, 0] + v[:, 1] * dv[:, 1]) / (cam.fx * cam.fx)
        J[:, k] = np.where(small, dtop, dtop / np.sqrt(safe) - 0.5 * top * dbottom / (safe * np.sqrt(safe)))
    return J


def retract(pose, delta):
    R, t = pose_parts(pose)
    b1, b2 = gm.sphere_basis(t)
    tn = t + delta[0] * b1 + delta[1] * b2
    return pose12(R @ gm.exp_se3([0.0, 0.0, 0.0, delta[2], delta[3], delta[4]])[0], tn / np.sqrt(tn @ tn))


def cost(cam, pose, A, B, a=A_HUBER):
    r = sampson(cam, pose, A, B)
    return 0.5 * np.sum(gm.huber(r * r, a)[1]), len(r)


def linearise(cam, pose, A, B, a=A_HUBER):
    r, J = sampson(cam, pose, A, B), jacobian(cam, pose, A, B)
    w = gm.huber(r * r, a)[0]
    return np.einsum("k,ki,kj->ij", w, J, J), np.einsum("k,ki,k->i", w, J, r)


def refine(cam, pose, A, B, a=A_HUBER, lambda_0=LAMBDA_0, ftol=FTOL, ptol=PTOL, decrease=DECREASE, increase=INCREASE,
           max_iterations=MAX_ITERATIONS):
    """the PnP block's LM driver over the five degrees of freedom.  trace: per iteration (cost_before, cost_candidate, accepted, lambda,
    |dE| / E / ftol, |delta|^2 / (ptol (state + ptol)))"""
    A, B = np.asarray(A, np.float64).reshape(-1, 2), np.asarray(B, np.float64).reshape(-1, 2)
    pose = np.array(pose, np.float64)
    lam = np.float64(lambda_0)
    E, nvalid = cost(cam, pose, A, B, a)
    E0, flags, it, lin, trace = E, 0, 0, None, []
    if nvalid == 0:
        flags = NO_VALID_RESIDUAL
    while it < max_iterations and flags == 0:
        if lin is None:
            lin = linearise(cam, pose, A, B, a)
        H, b = lin
        delta = gm.cholesky_solve(H + lam * np.diag(np.diag(H)), -b)
        it += 1
        if delta is None:
            trace.append((E, np.inf, 0, lam, np.inf, np.inf))
            lam = lam * increase
            continue
        cand = retract(pose, delta)
        En, _ = cost(cam, cand, A, B, a)
        state = pose[9:] @ pose[9:] + 1.0
        with np.errstate(all="ignore"):
            rf = np.float64(abs(E - En)) / E
            rp = (delta @ delta) / (ptol * (state + ptol))
        reason = FUNCTION_TOLERANCE if rf < ftol else 0
        accepted = bool(En < E)
        trace.append((E, En, int(accepted), lam, rf / ftol, rp))
        if accepted:
            if delta @ delta < ptol * (state + ptol):
                reason |= PARAMETER_TOLERANCE
            pose, E, lin = cand, En, None
            lam = lam / decrease
        else:
            lam = lam * increase
        flags = reason
    return Refinement(pose, it, flags, E0, E, trace)


# ---- the whole call

def estimate(cam, A, B, samples, threshold_px=0.5, min_matches=MIN_MATCHES, max_iterations=MAX_ITERATIONS, hyp=None, route="action"):
    """(Result, Hypotheses) of dsopp_hip_two_view_ransac_estimate; `hyp`: the hypotheses when they are known already"""
    A, B = np.asarray(A, np.float64).reshape(-1, 2), np.asarray(B, np.float64).reshape(-1, 2)
    t_ang = angular_threshold(cam, threshold_px)
    ok, fa, fb = match_mask(cam, A, B), bearings(cam, A), bearings(cam, B)
    matches = int(ok.sum())
    none = np.zeros(0, np.int64)
    empty = Hypotheses(np.zeros(0, np.int64), np.zeros((0, MAX_SOLUTIONS, 12)), np.zeros((0, MAX_SOLUTIONS), np.int64), np.zeros((0, MAX_SOLUTIONS, len(A))))
    stage0 = Refinement(IDENTITY.copy(), 0, 0, 0.0, 0.0, [])
    if matches < min_matches:
        return Result(matches, -1, -1, 0, 0, (stage0, stage0), IDENTITY.copy(), IDENTITY.copy(), IDENTITY.copy(), none, none, np.full(len(A), np.nan)), empty
    h = hyp if hyp is not None else hypotheses(cam, A, B, samples, t_ang, route)
    i, k, count = select(h.counts)
    if i < 0:
        return Result(matches, -1, -1, 0, 0, (stage0, stage0), IDENTITY.copy(), IDENTITY.copy(), IDENTITY.copy(), none, none, np.full(len(A), np.nan)), h
    pose_ransac = h.poses[i, k]
    ransac_inliers = np.flatnonzero(inlier_mask(h.distances[i, k], t_ang))
    first = refine(cam, pose_ransac, A[ransac_inliers], B[ransac_inliers], max_iterations=max_iterations)
    d = distances(*pose_parts(first.pose), fa, fb, ok)
    inliers = np.flatnonzero(inlier_mask(d, t_ang))
    second = refine(cam, first.pose, A[inliers], B[inliers], max_iterations=max_iterations)
    return Result(matches, i, k, count, len(inliers), (first, second), pose_ransac, first.pose, second.pose, ransac_inliers, inliers, d), h


def triangulate(cam, A, B, pose_a_b, pose_world_a, cos_threshold=COS_THRESHOLD):
    """(X_world (n, 3), keep (n,) bool, margins (n, 3): X_A.z and the two cosines) of triangulatePoints (triangulate_points.cpp:18-45)"""
    A, B = np.asarray(A, np.float64).reshape(-1, 2), np.asarray(B, np.float64).reshape(-1, 2)
    ok, fa, fb = match_mask(cam, A, B), bearings(cam, A), bearings(cam, B)
    R, t = pose_parts(np.asarray(pose_a_b, np.float64))
    Rw, tw = pose_parts(np.asarray(pose_world_a, np.float64))
    _, _, XA, XB = triangulate_pair(R, t, fa, fb)
    with np.errstate(all="ignore"):
        ca = (fa[:, 0] * XA[:, 0] + fa[:, 1] * XA[:, 1] + fa[:, 2] * XA[:, 2]) / np.sqrt(XA[:, 0] * XA[:, 0] + XA[:, 1] * XA[:, 1] + XA[:, 2] * XA[:, 2])
        cb = (fb[:, 0] * XB[:, 0] + fb[:, 1] * XB[:, 1] + fb[:, 2] * XB[:, 2]) / np.sqrt(XB[:, 0] * XB[:, 0] + XB[:, 1] * XB[:, 1] + XB[:, 2] * XB[:, 2])
        Xw = np.stack([Rw[k, 0] * XA[:, 0] + Rw[k, 1] * XA[:, 1] + Rw[k, 2] * XA[:, 2] + tw[k] for k in range(3)], axis=1)
        keep = ok & (XA[:, 2] > 0.0) & (ca > cos_threshold) & (cb > cos_threshold) & np.all(np.isfinite(Xw), axis=1) & np.isfinite(ca) & np.isfinite(cb)
    return Xw, keep, np.stack([XA[:, 2], ca, cb], axis=1)


def initialised(inliers, matches, ratio=0.6):
    """initializePoses' rule for step I (initialize_poses.cpp:37): false iff inliers < (size_t)(ratio * matches), with the truncation"""
    return not inliers < int(np.float64(ratio) * np.float64(matches))


# ---- the synthetic scene shared by the CPU and the GPU tests

CAM = Camera(448.0, 448.0, 320.0, 240.0, 640, 480)
_t = np.array([0.9, -0.1, 0.4])
TRUE_POSE = pose12(gm.exp_se3([0, 0, 0, 0.04, -0.06, 0.03])[0], _t / np.sqrt(_t @ _t))


def make_scene(n, seed, noise=0.3, outliers=0.3, outlier_sigma=15.0, cam=CAM, pose=TRUE_POSE, depth=(3.0, 12.0)):
    """n points at `depth` baselines in front of the first camera, seen by both inside the ROI; both observations carry N(0, noise) px, and
    a share `outliers` of the last frame's is displaced by N(0, outlier_sigma) px (kept inside the ROI by redrawing).  Returns (A, B)"""
    rng = np.random.default_rng(seed)
    R, t = pose_parts(pose)
    A, B = np.zeros((n, 2)), np.zeros((n, 2))
    for j in range(n):
        while True:
            a = np.array([rng.uniform(8.0, cam.width - 9.0), rng.uniform(8.0, cam.height - 9.0)])
            pa = np.array([(a[0] - cam.cx) / cam.fx, (a[1] - cam.cy) / cam.fy, 1.0]) * rng.uniform(depth[0], depth[1])
            pb = R.T @ (pa - t)
            b = np.array([cam.fx * pb[0] / pb[2] + cam.cx, cam.fy * pb[1] / pb[2] + cam.cy])
            if pb[2] > 0.5 and roi(cam, b - 4.0)[0] and roi(cam, b + 4.0)[0]:
                break
        A[j], B[j] = a, b
    An, Bn = A + noise * rng.standard_normal((n, 2)), B + noise * rng.standard_normal((n, 2))
    for j in np.flatnonzero(rng.random(n) < outliers):
        while True:
            o = Bn[j] + outlier_sigma * rng.standard_normal(2)
            if roi(cam, o)[0]:
                break
        Bn[j] = o
    return np.where(roi(cam, An)[:, None], An, A), np.where(roi(cam, Bn)[:, None], Bn, B)


def draw_samples(rng, n, count):
    return np.array([rng.choice(n, 5, replace=False) for _ in range(count)], np.int32).reshape(-1, 5)


# ---- a track to initialise, and its file

def make_initialisation_track(F=5, L=150, seed=80, noise=0.2, cam=CAM, pose=TRUE_POSE):
    """(cam, frames, landmarks) in tests/geometric_ba_model.py's form for initializePoses: F frames along the way from the identity to
    `pose`, none initialised and all at the identity; L landmarks without a position, each seen in the first and the last frame and in
    every frame between them whose ROI holds it, with N(0, noise) px on every observation.  The world is the first camera's frame"""
    rng = np.random.default_rng(seed)
    R, t = pose_parts(pose)
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2.0          # (small angles: the axis-angle vector to first order)
    poses = [pose12(gm.exp_se3(np.concatenate([np.zeros(3), w * f / (F - 1)]))[0], t * f / (F - 1)) for f in range(F)]
    frames = [dict(frame_id=20 + 3 * f, t_world_agent=IDENTITY.copy(), initialized=False) for f in range(F)]
    landmarks = []
    while len(landmarks) < L:
        a = np.array([rng.uniform(8.0, cam.width - 9.0), rng.uniform(8.0, cam.height - 9.0)])
        X = np.array([(a[0] - cam.cx) / cam.fx, (a[1] - cam.cy) / cam.fy, 1.0]) * rng.uniform(3.0, 12.0)
        proj = []
        for f in range(F):
            Rf, tf = pose_parts(poses[f])
            p = Rf.T @ (X - tf)
            q = np.array([cam.fx * p[0] / p[2] + cam.cx, cam.fy * p[1] / p[2] + cam.cy]) + noise * rng.standard_normal(2)
            if p[2] > 0.5 and roi(cam, q - 3.0)[0] and roi(cam, q + 3.0)[0]:
                proj.append((frames[f]["frame_id"], q))
        ids = [fid for fid, _ in proj]
        if frames[0]["frame_id"] in ids and frames[-1]["frame_id"] in ids:
            landmarks.append(dict(has=False, X=np.zeros(3), proj=proj))
    return tuple(cam), frames, landmarks


def write_initialisation_file(path, track, seed):
    """the input of dsopp_amd/host/example_initialize_poses.cpp: geometric_ba_model.write_track_file's records behind a header that ends
    in the seed of std::rand()"""
    import struct
    cam, frames, landmarks = track
    with open(path, "wb") as f:
        f.write(f"{cam[4]} {cam[5]} {len(frames)} {len(landmarks)} {seed}\n".encode())
        f.write(struct.pack("<4d", *cam[:4]))
        for fr in frames:
            f.write(struct.pack("<2i12d", fr["frame_id"], int(fr["initialized"]), *fr["t_world_agent"]))
        for lm in landmarks:
            f.write(struct.pack("<2i3d", int(lm["has"]), len(lm["proj"]), *lm["X"]))
            for fid, xy in lm["proj"]:
                f.write(struct.pack("<i2d", fid, *xy))
