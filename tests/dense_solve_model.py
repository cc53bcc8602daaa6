"""The criterion for the window's dense solve (calculateStep, problem.hpp:342-361): a componentwise backward error of a returned
step, computed in extended precision from the arrays the stage API hands out, with thresholds that follow from the algorithm.

    A = H_pp + lam diag(H_pp) + H_m - H_schur / (1 + lam)            (problem.hpp:347-351; the priors are inside H_pp, b_pp)
    g = b_pp - b_schur / (1 + lam) + b_m + H_m eps
    r = A x - g
    s_i = |H_pp,ii| (1 + lam) + |H_schur,ii| / (1 + lam) + |H_m,ii|
    t_i = |b_pp,i| + |b_schur,i| / (1 + lam) + |b_m,i| + sum_j |H_m,ij| |eps_j|
    omega(x) = max_i |r_i| / ( sqrt(s_i) sum_j sqrt(s_j) |x_j| + t_i )

omega is measured against the sizes of the terms that were ADDED, not against A: the cancellation in H_pp - H_schur (the monocular
scale gauge leaves the reduced system close to singular) does not enter it, and neither does the conditioning of A.  It is invariant
under a symmetric diagonal scaling of the system, so the 1e16 prior of a fixed frame does not swamp the other rows.  A row whose
denominator is 0 (a frame without any information: nothing was added to it) must have r_i == 0.

Thresholds, none of them taken from the code under test:
  cap(n)            2 (3 n + 8) u, n = K + 1, u = 2^-53.  (3 n + 1) u: Cholesky + two triangular solves (Higham, Accuracy and Stability
                    of Numerical Algorithms, Theorems 10.3 - 10.6 with | |R^T| |R| |_ij <= sqrt(a_ii a_jj) / (1 - gamma)); + 7 u: the
                    roundings of assembling A, g and -1 / (1 + lam); the factor 2: the device's pivot reciprocal is a Newton-refined
                    hardware estimate times a multiply, not a correctly rounded square root and divide (a stated allowance).
  working threshold 16 max(omega_lapack, u), omega_lapack = the same measure of a float64 LAPACK Cholesky solve of the same inputs
                    (lapack_step), computed inside each test case.  16 = four bits for another summation order and the
                    reciprocal-multiply.

Extended precision is numpy.longdouble where it has at least 60 mantissa bits (x87: epsilon 1.08e-19), mpmath at 40 digits elsewhere.
"""
import functools

import numpy as np

U = 2.0 ** -53
LAMBDAS = (1e-8, 1e-5, 1e-2, 1e2)
WINDOW_FRAMES = (2, 7, 8, 9, 12, 16)
WORKING_FACTOR = 16.0


def cap(K):
    return 2.0 * (3 * (K + 1) + 8) * U


class _LongDouble:
    name = "longdouble"

    @staticmethod
    def arr(a):
        return np.asarray(a, dtype=np.longdouble)

    @staticmethod
    def sqrt(a):
        return np.sqrt(a)


class _Mp:
    """object arrays of mpmath.mpf at 40 digits (hosts whose long double is the 53-bit double)"""
    name = "mpmath"

    @staticmethod
    def arr(a):
        import mpmath
        mpmath.mp.dps = 40
        a = np.asarray(a)
        out = np.empty(a.shape, dtype=object)
        for idx in np.ndindex(a.shape):
            v = a[idx]
            out[idx] = v if isinstance(v, mpmath.mpf) else mpmath.mpf(float(v))
        return out

    @staticmethod
    def sqrt(a):
        import mpmath
        out = np.empty(a.shape, dtype=object)
        for idx in np.ndindex(a.shape):
            out[idx] = mpmath.sqrt(a[idx])
        return out


def backend(force=None):
    if force == "mpmath" or (force is None and np.finfo(np.longdouble).eps > 2.0 ** -60):
        return _Mp
    return _LongDouble


class Measure:
    """omega and its rows: r (residual), den (denominator per row), ratio (|r_i| / den_i, 0 where den_i == 0), empty (den_i == 0)"""

    def __init__(self, r, den):
        self.r, self.den = r, den
        self.empty = np.array([d == 0 for d in den])
        ratio = np.zeros(len(den))
        for i in range(len(den)):
            if not self.empty[i]:
                ratio[i] = float(abs(r[i]) / den[i])
        self.ratio = ratio
        self.empty_rows_exact = all(r[i] == 0 for i in range(len(den)) if self.empty[i])
        self.omega = float(ratio.max()) if self.empty_rows_exact else np.inf


def measure(H_pp, b_pp, H_schur, b_schur, H_m, b_m, eps, lam, x, force=None):
    """the backward error of step x for the inputs of calculateStep (float64 arrays as the stage API returns them)"""
    B = backend(force)
    Hp, bp, Hs, bs, Hm, bm, e, xx = (B.arr(v) for v in (H_pp, b_pp, H_schur, b_schur, H_m, b_m, eps, x))
    one = B.arr(1.0)[()]
    lm = B.arr(float(lam))[()]
    opl = one + lm
    dHp, dHs, dHm = np.diagonal(Hp).copy(), np.diagonal(Hs).copy(), np.diagonal(Hm).copy()
    A = Hp + Hm - Hs / opl
    K = len(dHp)
    A[np.arange(K), np.arange(K)] += lm * dHp
    g = bp - bs / opl + bm + Hm @ e
    r = A @ xx - g
    s = np.abs(dHp) * opl + np.abs(dHs) / opl + np.abs(dHm)
    t = np.abs(bp) + np.abs(bs) / opl + np.abs(bm) + np.abs(Hm) @ np.abs(e)
    rs = B.sqrt(s)
    den = rs * (rs @ np.abs(xx)) + t
    return Measure(r, den)


def scale_terms(H_pp, H_schur, H_m, lam):
    """s of the criterion in float64 (D = diag(sqrt(s)) of the perturbation bound)"""
    return np.abs(np.diag(H_pp)) * (1 + lam) + np.abs(np.diag(H_schur)) / (1 + lam) + np.abs(np.diag(H_m))


def assemble64(H_pp, b_pp, H_schur, b_schur, H_m, b_m, eps, lam):
    """A, g of calculateStep in float64"""
    A = H_pp + H_m - H_schur / (1.0 + lam)
    K = len(b_pp)
    A[np.arange(K), np.arange(K)] += lam * np.diag(H_pp)
    g = b_pp - b_schur / (1.0 + lam) + b_m + H_m @ eps
    return A, g


def lapack_step(H_pp, b_pp, H_schur, b_schur, H_m, b_m, eps, lam):
    """the reference solve: assemble in float64, LAPACK Cholesky (potrf / potrs); only a system potrf rejects goes to the LU solve.
    Rows to which nothing was added (a frame without information: zero row, zero right-hand side) are no equations: their unknowns
    stay 0 and the rest is solved — what the device's zero-pivot guard and a rank-revealing L D L^T do with them."""
    from scipy.linalg import cho_factor, cho_solve
    A, g = assemble64(H_pp, b_pp, H_schur, b_schur, H_m, b_m, eps, lam)
    live = ~((np.abs(A).sum(axis=1) == 0) & (g == 0))
    x = np.zeros(len(g))
    Al, gl = A[np.ix_(live, live)], g[live]
    try:
        x[live] = cho_solve(cho_factor(Al, lower=True), gl)
    except np.linalg.LinAlgError:
        x[live] = np.linalg.solve(Al, gl)
    return x


def working_threshold(omega_lapack):
    return WORKING_FACTOR * max(omega_lapack, U)


def cholesky_step(A, g, block=8, recip_factor=1.0, skip_rhs_update_of_block=None):
    """Plain unblocked Cholesky of the augmented system [[A, .], [g^T, 0]] in float64 and the back substitution, written the way the
    device does it (l_ik = c_ik * inv_k with inv_k the pivot's inverse square root, x_k = y_k * inv_k), with two deliberate faults for the
    tests of the criterion: `recip_factor` multiplies every pivot reciprocal; `skip_rhs_update_of_block` = kb leaves the right-hand-side
    row (row K of L) without the update by block column kb (columns block * kb ...) — what a panel loop that misses the last row does."""
    K = len(g)
    L = np.zeros((K + 1, K + 1))
    L[:K, :K] = np.tril(A)
    L[K, :K] = g
    inv = np.zeros(K)
    for k in range(K):
        d = L[k, k]
        inv[k] = (1.0 / np.sqrt(d)) * recip_factor if d > 0 else 0.0
        L[k:, k] *= inv[k]
        col = L[k + 1:, k].copy()
        if skip_rhs_update_of_block is not None and k // block == skip_rhs_update_of_block:
            col[-1] = 0.0
        L[k + 1:, k + 1:K] -= np.outer(col, L[k + 1:K, k])   # (the strict upper triangle takes the update too: never read)
    y = L[K, :K].copy()
    x = np.zeros(K)
    for k in range(K - 1, -1, -1):
        x[k] = y[k] * inv[k]
        y[:k] -= L[k, :k] * x[k]
    return x


# ---- the windows of the dense-solve tests (shared by the CPU and the GPU file: built once per process)

@functools.lru_cache(maxsize=None)
def make_case_window(F, flip_last=False):
    """320 x 240, 80 landmarks per frame, seed 100 + F; from 13 keyframes on the slower camera of test_window_at_capacity (16 keyframes
    of the default motion leave the scene).  flip_last: the last keyframe looks the other way (no residual into or out of it)."""
    from dsopp_amd import synthetic as syn
    base = syn.BASE_MOTION.copy()
    if F >= 13:
        syn.BASE_MOTION[:] = base * 0.4
    try:
        win = syn.make_window(num_frames=F, num_points=80 * F, width=320, height=240, seed=100 + F)
    finally:
        syn.BASE_MOTION[:] = base
    if flip_last:
        flip = np.eye(4)
        flip[:3, :3] = np.diag([-1.0, 1.0, -1.0])     # 180 degrees about y
        win.frames[-1].T_w_c_init = win.frames[-1].T_w_c_init @ flip
    return win


@functools.lru_cache(maxsize=None)
def make_marginal_window(n_frames):
    from dsopp_amd import synthetic as syn
    if n_frames == 5:    # the window of tests/test_marginalization.py
        return syn.make_window(num_frames=5, num_points=300, width=320, height=240, seed=21)
    return syn.make_window(num_frames=n_frames, num_points=80 * n_frames, width=320, height=240, seed=100 + n_frames)


def read_inputs(w, frame_ids):
    """(H_pp, b_pp, H_schur, b_schur, H_m, b_m, eps) of a linearised window, oracle or device"""
    H_pp, b_pp, H_schur, b_schur = w.get_system()
    H_m, b_m, _ = w.get_marginalized()
    eps = np.concatenate([w.get_frame_state(fid)[2] for fid in frame_ids])
    return H_pp, b_pp, H_schur, b_schur, H_m, b_m, eps


def check_step(inputs, lam, x, label=""):
    """asserts cap and working threshold for step x; returns (omega, omega_lapack, Measure)"""
    K = len(x)
    assert np.all(np.isfinite(x)), label
    m = measure(*inputs, lam, x)
    ml = measure(*inputs, lam, lapack_step(*inputs, lam))
    assert m.empty_rows_exact, (label, "a row nothing was added to has a residual")
    assert m.omega <= cap(K), (label, lam, m.omega, cap(K))
    assert m.omega <= working_threshold(ml.omega), (label, lam, m.omega, ml.omega, working_threshold(ml.omega))
    return m.omega, ml.omega, m
