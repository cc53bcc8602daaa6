"""A plain NumPy statement of ONE linearisation of the two-frame direct image alignment (DESIGN.md "pose aligner"; SURVEY.md hot loops
E, F), written from the maths, and the generators of the cases the aligner's edge tests run (tests/test_align_model.py checks the model
and guards the generators on the CPU, tests/test_gpu_align_edges.py runs the device code against both).

The maths.  A reference point (u, v, rho) — pixel and inverse depth — is the homogeneous point x = (u, v, 1, rho).  With the pinhole
matrices K_r, K_t and T_target_reference = [R | t]:

    P = [R | t] Kinv_r x        a point ALONG the target ray (the true point is P / rho), Kinv_r = the 4 x 4 extension of K_r^-1
    p = K_t P,  (tu, tv) = (p_x, p_y) / p_z,  p_z = P_z
    valid  <=>  -1e-4 < rho < 1010  and  (u, v) in the reference ROI  and  p_z > 0  and  (tu, tv) in the target ROI
                and  mask[round(tv), round(tu)] != 0                        ROI: 4 <= x <= W - 5, 4 <= y <= H - 5
    r = (I_t(tu, tv) - b_t) - s (I_r - b_r),   s = (e_t / e_r) exp(a_t - a_r),   (a_t, b_t) = target affine + candidate increment
    I_t, dI_t/dx, dI_t/dy: the bilinear blend of the stored (I, Ix, Iy) triplets of the texel cell (floor(tu), floor(tv))
    Huber: r^2 > sigma^2 ? (w = sigma / |r|, e = sigma |r| - sigma^2 / 2) : (w = 1, e = r^2 / 2)

The pose is perturbed on the LEFT, T <- exp(eps) T with eps = (translation, rotation): dP / d eps = [rho I | -[P]x].  The reference's
normal equations use the row

    d = (-dr / d eps (6), +dr / d a_t, +dr / d b_t) = (-(Ix, Iy) dpi/dP dP/d eps, -s (I_r - b_r), -1)

and the update T <- exp(x[:6]) T, (a, b) <- (a, b) - x[6:] for (H + lambda diag H) x = b; H = sum w d d^T + diag(0 .. 0, reg_a, reg_b),
b = sum w d r + (0 .. 0, reg_a a_t, reg_b b_t), energy = sum e + (reg_a a_t^2 + reg_b b_t^2) / 2.

Precision: the per-point stage runs in `dtype` (numpy.float64, or numpy.float32 to MEASURE what single precision does to it: inputs,
the two 3 x 4 matrices, the bilinear sample, residual and row are then float32 values; the Huber decision and all sums are not), every sum
is taken in numpy.longdouble.
"""
import functools

import numpy as np

LD = np.longdouble
BORDER = 4.0
IDEPTH_MIN, IDEPTH_MAX = -1e-4, 1.0 / 0.001 + 1e1
REASONS = ("valid", "idepth", "reference_roi", "behind", "target_roi", "mask")   # the FIRST test a point fails


def se3_exp(xi):
    """exp of the twist (translation part, rotation vector) as a 4 x 4 matrix (Rodrigues; series below 1e-8 rad)"""
    xi = np.asarray(xi, dtype=np.float64)
    w = xi[3:]
    th = float(np.linalg.norm(w))
    Om = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-8:
        A, B, Cc = 1.0 - th * th / 6, 0.5 - th * th / 24, 1.0 / 6 - th * th / 120
    else:
        A, B, Cc = np.sin(th) / th, (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + A * Om + B * Om @ Om
    T[:3, 3] = (np.eye(3) + B * Om + Cc * Om @ Om) @ xi[:3]
    return T


def bilinear(planes, x, y, dtype=np.float64):
    """bilinear blend of the (I, Ix, Iy) triplets at the non-integer positions (x, y): n x 3.  Positions must have their cell inside."""
    planes = np.asarray(planes)
    x, y = np.asarray(x, dtype=dtype), np.asarray(y, dtype=dtype)
    ix, iy = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    dx, dy = (x - ix.astype(dtype))[:, None], (y - iy.astype(dtype))[:, None]
    one = dtype(1)
    p = planes.astype(dtype)
    return ((one - dx) * (one - dy) * p[iy, ix] + dx * (one - dy) * p[iy, ix + 1] + (one - dx) * dy * p[iy + 1, ix] + dx * dy * p[iy + 1, ix + 1])


def _inside(x, y, W, H, dtype):
    return (x >= dtype(BORDER)) & (y >= dtype(BORDER)) & (x <= dtype(W - BORDER - 1)) & (y <= dtype(H - BORDER - 1))


def reference_intensity(ref_planes, u, v, dtype=np.float64):
    """the bilinear sample of the reference image at the points; 0 for a point outside the reference ROI (it is never used)"""
    H, W = np.asarray(ref_planes).shape[:2]
    u, v = np.asarray(u, dtype=dtype), np.asarray(v, dtype=dtype)
    with np.errstate(invalid="ignore"):
        ok = _inside(u, v, W, H, dtype)
    out = np.zeros(len(u), dtype=dtype)
    if ok.any():
        out[ok] = bilinear(ref_planes, u[ok], v[ok], dtype)[:, 0]
    return out.astype(np.float64)


def _matrices(ref_intr, tgt_intr, T_tr):
    fx, fy, cx, cy = (float(x) for x in ref_intr)
    Kinv = np.array([[1 / fx, 0, -cx / fx, 0], [0, 1 / fy, -cy / fy, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    U = np.asarray(T_tr, dtype=np.float64)[:3, :] @ Kinv                       # P = U x
    Kt = np.array([[tgt_intr[0], 0, tgt_intr[2]], [0, tgt_intr[1], tgt_intr[3]], [0, 0, 1.0]])
    return U, Kt @ U                                                           # p = M x


def linearize(u, v, idepth, intensity, tgt_planes, tgt_mask, ref_intr, ref_size, tgt_intr, T_tr, ref_exposure=1.0, ref_ab=(0.0, 0.0),
              tgt_exposure=1.0, tgt_ab=(0.0, 0.0), cand_ab=(0.0, 0.0), sigma_huber=9.0, affine_reg=(0.0, 0.0), dtype=np.float64):
    """One linearisation at the state (T_tr 4 x 4, cand_ab).  `intensity`: the points' reference intensities (reference_intensity()).
    Returns a dict: per point tu, tv, pz, reason (index into REASONS; 0 = valid), valid, sample (I, Ix, Iy of the target), residual, weight,
    row (n x 8), energy term; the sums
    H (8 x 8, prior folded in), b (8), energy (prior included), n_valid — float64 values of long double sums."""
    S = dtype
    tgt_planes = np.asarray(tgt_planes)
    Ht, Wt = tgt_planes.shape[:2]
    Wr, Hr = ref_size
    n = len(u)
    U64, M64 = _matrices(ref_intr, tgt_intr, T_tr)
    U, M = U64.astype(S), M64.astype(S)
    x = np.stack([np.asarray(u, dtype=S), np.asarray(v, dtype=S), np.ones(n, dtype=S), np.asarray(idepth, dtype=S)], axis=1)
    iref = np.asarray(intensity, dtype=S)
    a_t, b_t = float(tgt_ab[0]) + float(cand_ab[0]), float(tgt_ab[1]) + float(cand_ab[1])
    s = S((tgt_exposure / ref_exposure) * np.exp(a_t - float(ref_ab[0])))
    with np.errstate(all="ignore"):
        p = x @ M.T
        P = x @ U.T
        tu, tv = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
        reason = np.zeros(n, dtype=np.int64)

        def fail(cond, code):
            reason[(reason == 0) & cond] = code
        fail(~((x[:, 3] > S(IDEPTH_MIN)) & (x[:, 3] < S(IDEPTH_MAX))), 1)
        fail(~_inside(x[:, 0], x[:, 1], Wr, Hr, S), 2)
        fail(~(p[:, 2] > 0), 3)
        fail(~_inside(tu, tv, Wt, Ht, S), 4)
        ok = reason == 0
        if tgt_mask is not None:
            m = np.asarray(tgt_mask)
            rx, ry = np.floor(tu[ok] + S(0.5)).astype(np.int64), np.floor(tv[ok] + S(0.5)).astype(np.int64)   # round(): positions are positive
            bad = np.zeros(n, dtype=bool)
            bad[ok] = m[ry, rx] == 0
            fail(bad, 5)
            ok = reason == 0
    sample = np.zeros((n, 3), dtype=S)
    sample[ok] = bilinear(tgt_planes, tu[ok], tv[ok], S)
    right = s * (iref - S(ref_ab[1]))
    res = ((sample[:, 0] - S(b_t)) - right).astype(np.float64)
    row = np.zeros((n, 8), dtype=S)
    if ok.any():
        Pv, rho = P[ok], x[ok, 3]
        Z = Pv[:, 2]
        fxt, fyt = S(tgt_intr[0]), S(tgt_intr[1])
        # d pi / d P (2 x 3) and d P / d eps = [rho I | -[P]x] (3 x 6), per point
        dpi = np.zeros((len(Z), 2, 3), dtype=S)
        dpi[:, 0, 0] = fxt / Z
        dpi[:, 0, 2] = -fxt * Pv[:, 0] / (Z * Z)
        dpi[:, 1, 1] = fyt / Z
        dpi[:, 1, 2] = -fyt * Pv[:, 1] / (Z * Z)
        dP = np.zeros((len(Z), 3, 6), dtype=S)
        for k in range(3):
            dP[:, k, k] = rho
        dP[:, 0, 4], dP[:, 0, 5] = Pv[:, 2], -Pv[:, 1]
        dP[:, 1, 3], dP[:, 1, 5] = -Pv[:, 2], Pv[:, 0]
        dP[:, 2, 3], dP[:, 2, 4] = Pv[:, 1], -Pv[:, 0]
        duv = np.einsum("nij,njk->nik", dpi, dP)
        row[ok, :6] = -(sample[ok, 1, None] * duv[:, 0, :] + sample[ok, 2, None] * duv[:, 1, :])
        row[ok, 6] = -right[ok]
        row[ok, 7] = S(-1)
    row = row.astype(np.float64)
    lin = res * res > sigma_huber * sigma_huber
    with np.errstate(divide="ignore", invalid="ignore"):
        wgt = np.where(ok, np.where(lin, sigma_huber / np.abs(res), 1.0), 0.0)
    en = np.where(ok, np.where(lin, sigma_huber * np.abs(res) - 0.5 * sigma_huber ** 2, 0.5 * res * res), 0.0)
    rl, wl, dl = res.astype(LD), wgt.astype(LD), row.astype(LD)
    Hs = np.einsum("n,ni,nj->ij", wl[ok], dl[ok], dl[ok]) if ok.any() else np.zeros((8, 8), dtype=LD)
    bs = np.einsum("n,ni,n->i", wl[ok], dl[ok], rl[ok]) if ok.any() else np.zeros(8, dtype=LD)
    Hs[6, 6] += LD(affine_reg[0])
    Hs[7, 7] += LD(affine_reg[1])
    bs[6] += LD(affine_reg[0]) * LD(a_t)
    bs[7] += LD(affine_reg[1]) * LD(b_t)
    energy = en.astype(LD).sum() + (LD(a_t) * LD(affine_reg[0]) * LD(a_t) + LD(b_t) * LD(affine_reg[1]) * LD(b_t)) / 2
    return dict(tu=tu.astype(np.float64), tv=tv.astype(np.float64), pz=p[:, 2].astype(np.float64), reason=reason, valid=ok, residual=res,
                weight=wgt, row=row, energy_terms=en, sample=sample.astype(np.float64), linear=lin & ok, H=Hs.astype(np.float64), b=bs.astype(np.float64), energy=float(energy),
                n_valid=int(ok.sum()))


def lm_first_step(H, b, lam, T_tr, cand_ab=(0.0, 0.0)):
    """(H + lambda diag H) x = b; returns the candidate exp(x[:6]) T_tr, the candidate affine increment cand_ab - x[6:], and x"""
    A = np.array(H, dtype=np.float64)
    A[np.diag_indices(8)] += lam * np.diag(H)
    x = np.linalg.solve(A, np.asarray(b, dtype=np.float64))
    return se3_exp(x[:6]) @ np.asarray(T_tr, dtype=np.float64), np.asarray(cand_ab, dtype=np.float64) - x[6:], x


def margins(lin, ref_size, tgt_size, sigma_huber, u, v, idepth, masked):
    """per point: the distance of the quantities the decisions are taken on from every decision edge it reaches (a point that has failed a
    test is not asked the later ones) — idepth bounds, reference ROI, p_z = 0, target ROI, the .5 rounding of the mask lookup (masked
    cases only), |r| = sigma.  n x 6, unreached entries +inf."""
    n = len(u)
    out = np.full((n, 6), np.inf)
    u, v, idepth = (np.asarray(a, dtype=np.float64) for a in (u, v, idepth))
    Wr, Hr = ref_size
    Wt, Ht = tgt_size
    r = lin["reason"]
    out[:, 0] = np.minimum(np.abs(idepth - IDEPTH_MIN), np.abs(idepth - IDEPTH_MAX))
    reach = (r == 0) | (r >= 2)
    out[reach, 1] = np.min(np.abs(np.stack([u - BORDER, Wr - BORDER - 1 - u, v - BORDER, Hr - BORDER - 1 - v])), axis=0)[reach]
    reach = (r == 0) | (r >= 3)
    out[reach, 2] = np.abs(lin["pz"])[reach]
    reach = (r == 0) | (r >= 4)
    tu, tv = lin["tu"], lin["tv"]
    out[reach, 3] = np.min(np.abs(np.stack([tu - BORDER, Wt - BORDER - 1 - tu, tv - BORDER, Ht - BORDER - 1 - tv])), axis=0)[reach]
    reach = (r == 0) | (r >= 5)
    if masked:
        out[reach, 4] = np.minimum(np.abs(tu - np.floor(tu) - 0.5), np.abs(tv - np.floor(tv) - 0.5))[reach]
    reach = r == 0
    out[reach, 5] = np.abs(np.abs(lin["residual"]) - sigma_huber)[reach]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# one LM iteration as the solvers report it with max_iterations = 1 (levenberg_marquardt_algorithm.hpp:77-128): the system is the initial
# state's, energy / n_valid / pose / affine are the candidate's when it was accepted (lower energy, any valid residual) and the initial
# state's otherwise
# ---------------------------------------------------------------------------------------------------------------------------------------
def first_iteration(c, dtype=np.float64, intensity=None):
    """c: a case of this module.  Returns dict(H, b, energy0, n0, energy, n_valid, accepted, T_tr, T_w_target (4 x 4), affine, x, lin0, lin1)"""
    kw = dict(tgt_planes=c["tgt_planes"], tgt_mask=c["mask"], ref_intr=c["intr"], ref_size=c["size"], tgt_intr=c["tgt_intr"], ref_exposure=c["e_ref"],
              ref_ab=c["ab_ref"], tgt_exposure=c["e_tgt"], tgt_ab=c["ab_tgt"], sigma_huber=c["sigma"], affine_reg=c["reg"], dtype=dtype)
    inten = c["intensity"] if intensity is None else intensity
    T0 = np.linalg.inv(c["T_w_tgt"]) @ c["T_w_ref"]
    l0 = linearize(c["u"], c["v"], c["idepth"], inten, T_tr=T0, **kw)
    out = dict(H=l0["H"], b=l0["b"], energy0=l0["energy"], n0=l0["n_valid"], lin0=l0, lin1=None, accepted=False, T_tr=T0, affine=np.array(c["ab_tgt"], dtype=np.float64),
               energy=l0["energy"], n_valid=l0["n_valid"], x=np.zeros(8))
    if l0["n_valid"] > 0 and np.all(np.isfinite(l0["H"])):
        try:
            T1, ab1, x = lm_first_step(l0["H"], l0["b"], c["lambda0"], T0)
        except np.linalg.LinAlgError:
            T1 = None
        if T1 is not None and np.all(np.isfinite(x)):
            l1 = linearize(c["u"], c["v"], c["idepth"], inten, T_tr=T1, cand_ab=ab1, **kw)
            out.update(lin1=l1, x=x)
            if l1["n_valid"] > 0 and l1["energy"] < l0["energy"]:
                out.update(accepted=True, T_tr=T1, affine=np.asarray(c["ab_tgt"]) + ab1, energy=l1["energy"], n_valid=l1["n_valid"])
    out["T_w_target"] = c["T_w_ref"] @ np.linalg.inv(out["T_tr"])
    return out


def lm_solve(c, dtype=np.float64, intensity=None, max_iterations=50, function_tolerance=1e-5, parameter_tolerance=1e-5):
    """the whole Levenberg-Marquardt loop around linearize() (levenberg_marquardt_algorithm.hpp:77-128 with the aligner's options: lambda
    halves on accept and doubles on reject, a rejected step keeps the system).  Returns dict(T_w_target 4 x 4, affine, iterations, n_valid,
    energy, trace); trace: per iteration (|de| / e / function_tolerance, |x|^2 / (parameter_tolerance (|ab|^2 + parameter_tolerance)),
    accepted) — the quantities the termination decisions compare with 1."""
    kw = dict(tgt_planes=c["tgt_planes"], tgt_mask=c["mask"], ref_intr=c["intr"], ref_size=c["size"], tgt_intr=c["tgt_intr"], ref_exposure=c["e_ref"],
              ref_ab=c["ab_ref"], tgt_exposure=c["e_tgt"], tgt_ab=c["ab_tgt"], sigma_huber=c["sigma"], affine_reg=c["reg"], dtype=dtype)
    inten = c["intensity"] if intensity is None else intensity
    T, ab, lam = np.linalg.inv(c["T_w_tgt"]) @ c["T_w_ref"], np.zeros(2), c["lambda0"]
    cur = linearize(c["u"], c["v"], c["idepth"], inten, T_tr=T, cand_ab=ab, **kw)
    system, energy, n_valid, converged, iterations, trace = cur, cur["energy"], cur["n_valid"], False, 0, []
    while iterations < max_iterations and not converged and n_valid > 0:
        iterations += 1
        T1, ab1, x = lm_first_step(system["H"], system["b"], lam, T, ab)
        nxt = linearize(c["u"], c["v"], c["idepth"], inten, T_tr=T1, cand_ab=ab1, **kw)
        if nxt["n_valid"] == 0:
            break
        a0 = np.asarray(c["ab_tgt"]) + ab
        rf = abs(energy - nxt["energy"]) / energy / function_tolerance
        rp = float(x @ x) / (parameter_tolerance * (float(a0 @ a0) + parameter_tolerance))
        accepted = nxt["energy"] < energy
        trace.append((rf, rp, accepted))
        converged = converged or rf < 1
        if accepted:
            converged = converged or rp < 1
            T, ab, energy, n_valid, system, lam = T1, ab1, nxt["energy"], nxt["n_valid"], nxt, lam / 2
        else:
            lam *= 2
    return dict(T_w_target=c["T_w_ref"] @ np.linalg.inv(T), affine=np.asarray(c["ab_tgt"]) + ab, iterations=iterations, n_valid=n_valid, energy=energy,
                trace=trace)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the cases.  Frames: two views of the analytic scene of dsopp_amd.synthetic; planes: level 0 of the frame's pyramid (the 8-bit image
# and its central differences, exact in float32 as well); points: non-integer reference positions with the scene's inverse depth
# ---------------------------------------------------------------------------------------------------------------------------------------
SIZE = (160, 120)
F64_MARGIN = 1e-6      # every case: no decision of the first linearisation within this of its edge
# float32 cases: a target coordinate (<= 160) carries ~10 roundings of 2^-24 relative, i.e. ~1e-4 px, a residual (<= 255) likewise ~1e-4:
# decisions closer than 1e-3 to their edge may legitimately fall either way in single precision, so those cases keep no such point, at the
# initial state and at the first candidate
F32_MARGIN = 1e-3
HUBER_SIGMA = 4.5      # the "small sigma" of the Huber case: 30 % .. 70 % of its valid residuals are on the linear branch (guarded)


@functools.lru_cache(maxsize=None)
def frames(size=SIZE, seed=11):
    """(window, reference planes, target planes) — planes H x W x 3 float64 of level 0"""
    from dsopp_amd import synthetic as syn
    win = syn.make_window(num_frames=2, num_points=16, width=size[0], height=size[1], seed=seed)
    pr, pt = (syn.pixelinfo_from_plane(f.image_u8.astype(np.float64)) for f in win.frames)
    pr.setflags(write=False)
    pt.setflags(write=False)
    return win, pr, pt


def _case(u, v, idepth, mask=None, sigma=None, reg=None, e_ref=1.0, ab_ref=(0.0, 0.0), e_tgt=1.0, ab_tgt=(0.0, 0.0), name="", target=None, tgt_intr=None):
    """target: (8-bit image, planes, initial T_world_target) of another target view than the window's second frame"""
    win, pr, pt = frames()
    fr, ft = win.frames
    image_tgt, pt, T_w_tgt = (ft.image_u8, pt, ft.T_w_c_init) if target is None else target
    c = dict(name=name, u=np.ascontiguousarray(u, dtype=np.float64), v=np.ascontiguousarray(v, dtype=np.float64),
             idepth=np.ascontiguousarray(idepth, dtype=np.float64), ref_planes=pr, tgt_planes=pt, mask=mask, size=SIZE,
             intr=np.asarray(win.scene.intrinsics, dtype=np.float64), T_w_ref=fr.T_w_c_gt.copy(), T_w_tgt=T_w_tgt.copy(),
             tgt_intr=np.asarray(win.scene.intrinsics if tgt_intr is None else tgt_intr, dtype=np.float64),
             e_ref=e_ref, ab_ref=np.array(ab_ref, dtype=np.float64), e_tgt=e_tgt, ab_tgt=np.array(ab_tgt, dtype=np.float64),
             sigma=DEFAULT_SIGMA if sigma is None else sigma, reg=DEFAULT_REG if reg is None else tuple(reg), lambda0=1.0 / 1e2,
             image_ref=fr.image_u8, image_tgt=image_tgt)
    c["intensity"] = reference_intensity(pr, c["u"], c["v"])
    return c


DEFAULT_SIGMA = 20.0          # sigma_huber_loss and affine_brightness_regularizer of default_align_options (test_align_model.py asserts both)
DEFAULT_REG = (1e12, 1e8)


def options_kw(c, **kw):
    """the keyword arguments of default_align_options (library and oracle alike) of a case"""
    return dict(sigma_huber_loss=c["sigma"], affine_brightness_regularizer=tuple(c["reg"]), **kw)


def random_points(n, seed, pool=None):
    """n non-integer reference positions inside the ROI with the scene's inverse depth there (+- 1 %); `pool`: draw them with replacement
    from the first `pool` positions instead"""
    win, _, _ = frames()
    W, H = SIZE
    rng = np.random.default_rng(seed)
    m = n if pool is None else pool
    u = rng.uniform(BORDER + 0.01, W - BORDER - 1.01, m)
    v = rng.uniform(BORDER + 0.01, H - BORDER - 1.01, m)
    depth = win.frames[0].depth
    idepth = (1.0 / depth[np.rint(v).astype(int), np.rint(u).astype(int)]) * (1 + rng.uniform(-0.01, 0.01, m))
    if pool is not None:
        k = rng.integers(0, pool, n)
        u, v, idepth = u[k], v[k], idepth[k]
    return u, v, idepth


def _keep_clear(c, margin, both_states):
    """drop the points of case c whose decisions come within `margin` of an edge (at the first candidate too when both_states)"""
    fi = first_iteration(c)
    mg = margins(fi["lin0"], c["size"], c["size"], c["sigma"], c["u"], c["v"], c["idepth"], c["mask"] is not None).min(axis=1)
    if both_states and fi["lin1"] is not None:
        mg = np.minimum(mg, margins(fi["lin1"], c["size"], c["size"], c["sigma"], c["u"], c["v"], c["idepth"], c["mask"] is not None).min(axis=1))
    keep = mg >= margin
    for k in ("u", "v", "idepth", "intensity"):
        c[k] = np.ascontiguousarray(c[k][keep])
    return c


def partial_mask():
    """a target mask with a masked rectangle and a masked band: part of the projections land on zeros"""
    W, H = SIZE
    m = np.ones((H, W), dtype=np.uint8)
    m[30:70, 40:90] = 0
    m[:, 120:131] = 0
    return m


def checkerboard_mask():
    W, H = SIZE
    yy, xx = np.mgrid[0:H, 0:W]
    return ((xx + yy) % 2).astype(np.uint8)


PHOTOMETRIC = dict(e_ref=0.8, ab_ref=(0.02, 1.5), e_tgt=1.1, ab_tgt=(-0.01, -0.7))


@functools.lru_cache(maxsize=None)
def case(name, n=1500, f32=False):
    """the named cases of the aligner tests; f32: cleared of points within F32_MARGIN of a decision edge (see above)"""
    margin, both = (F32_MARGIN, True) if f32 else (F64_MARGIN, False)
    seed = dict(default=1, photometric=2, weak_prior=3, mask=4, huber=5, cameras=6)[name]
    u, v, idp = random_points(n + (n // 8 if f32 else 0), seed)
    kw = dict(default={}, photometric=PHOTOMETRIC, weak_prior=dict(reg=(1e1, 1e-3), **PHOTOMETRIC), mask=dict(mask=partial_mask()),
              huber=dict(sigma=HUBER_SIGMA), cameras=dict(tgt_intr=frames()[0].scene.intrinsics * [1.03, 0.98, 1, 1] + [0, 0, 1.5, -2.25]))[name]
    c = _keep_clear(_case(u, v, idp, name=name, **kw), margin, both)
    for k in ("u", "v", "idepth", "intensity"):
        c[k] = np.ascontiguousarray(c[k][:n])
    return c


def reject_case():
    """the default case from a start whose first (practically undamped) step is rejected: see test_model_reject_branch_equals_oracle"""
    c = dict(case("default"))
    c.update(name="reject", reg=(1e-3, 1e-3), ab_tgt=np.array([-2.0, 0.0]), lambda0=1e-12)
    return c


def backproject(tu, tv, idepth, c):
    """reference positions whose projection into the target at the case's initial pose is (tu, tv), for points of inverse depth `idepth`
    (as seen from the REFERENCE).  Solved by a few Newton steps on the model's own projection."""
    T_tr = np.linalg.inv(c["T_w_tgt"]) @ c["T_w_ref"]
    _, M = _matrices(c["intr"], c["tgt_intr"], T_tr)
    tu, tv, idepth = (np.asarray(a, dtype=np.float64) for a in (tu, tv, idepth))
    # p ~ M (u, v, 1, rho): two linear equations in (u, v) per point
    A = np.stack([np.stack([M[0, 0] - tu * M[2, 0], M[0, 1] - tu * M[2, 1]], axis=1), np.stack([M[1, 0] - tv * M[2, 0], M[1, 1] - tv * M[2, 1]], axis=1)], axis=1)
    rhs = -np.stack([(M[0, 2] - tu * M[2, 2]) + (M[0, 3] - tu * M[2, 3]) * idepth, (M[1, 2] - tv * M[2, 2]) + (M[1, 3] - tv * M[2, 3]) * idepth], axis=1)
    uv = np.linalg.solve(A, rhs[..., None])[..., 0]
    return uv[:, 0], uv[:, 1]


@functools.lru_cache(maxsize=None)
def forward_target():
    """a target view half a metre FORWARD of the reference: the image is magnified by ~9 %, so the whole border of the target ROI is seen
    from inside the reference ROI, and points nearer than half a metre to the reference lie behind the target camera"""
    from dsopp_amd import synthetic as syn
    win, _, _ = frames()
    T_gt = syn.se3_exp(np.array([0.05, 0.01, 0.5, 0.004, 0.012, 0.003]))
    img, _ = win.scene.render(T_gt)
    u8 = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    planes = syn.pixelinfo_from_plane(u8.astype(np.float64))
    planes.setflags(write=False)
    return u8, planes, T_gt @ syn.se3_exp(np.array([0.01, -0.008, 0.012, 0.003, -0.002, 0.004]))


@functools.lru_cache(maxsize=None)
def edge_case():
    """every validity decision of the sweep from both sides, against a checkerboard target mask:
      * target projections 0.01 / 0.3 px inside and outside each of the four target ROI bounds (back-projected target pixels);
      * points behind the target camera (forward_target(): nearer to the reference than the target's advance);
      * inverse depths just inside and just outside (-1e-4, 1010);
      * reference positions just inside and just outside the reference ROI;
      * projections on both sides of .5 in x and in y (the mask's rounding), on masked and unmasked pixels.
    Every group holds at least six points per side."""
    W, H = SIZE
    win, pr, pt = frames()
    rng = np.random.default_rng(77)
    tgt = forward_target()
    base = _case(np.zeros(0), np.zeros(0), np.zeros(0), mask=checkerboard_mask(), name="edges", target=tgt)
    us, vs, ids = [], [], []
    k = 8
    # target ROI: left / right / top / bottom, inside and outside
    for d in (0.01, 0.3, -0.01, -0.3):     # d > 0: inside
        along_x, along_y = rng.uniform(20, W - 20, k), rng.uniform(20, H - 20, k)
        for tu, tv in ((np.full(k, BORDER + d), along_y), (np.full(k, W - BORDER - 1 - d), along_y), (along_x, np.full(k, BORDER + d)),
                       (along_x, np.full(k, H - BORDER - 1 - d))):
            rho = rng.uniform(0.12, 0.2, k)
            bu, bv = backproject(tu, tv, rho, base)
            us.append(bu), vs.append(bv), ids.append(rho)
    # the mask's rounding: projections at (integer + .5 -+ 0.02) in x (y well inside a cell) and in y
    for off in (0.48, 0.52):
        cx, cy = rng.integers(20, W - 20, 3 * k).astype(np.float64), rng.integers(20, H - 20, 3 * k).astype(np.float64)
        for tu, tv in ((cx + off, cy + rng.uniform(0.1, 0.4, 3 * k)), (cx + rng.uniform(0.6, 0.9, 3 * k), cy + off)):
            rho = rng.uniform(0.12, 0.2, 3 * k)
            bu, bv = backproject(tu, tv, rho, base)
            us.append(bu), vs.append(bv), ids.append(rho)
    # inverse depth bounds (a far point, rho ~ 0, projects by the rotation alone: inside; rho ~ 1010 is 1 mm in front of the reference)
    for rho in (IDEPTH_MIN + 2e-6, IDEPTH_MIN - 2e-6, IDEPTH_MAX - 2e-3, IDEPTH_MAX + 2e-3):
        us.append(rng.uniform(30, W - 30, k)), vs.append(rng.uniform(30, H - 30, k)), ids.append(np.full(k, rho))
    # reference ROI, both sides of every bound
    for d in (0.001, -0.001):
        a, b = rng.uniform(30, W - 30, k), rng.uniform(30, H - 30, k)
        for ru, rv in ((np.full(k, BORDER + d), b), (np.full(k, W - BORDER - 1 - d), b), (a, np.full(k, BORDER + d)), (a, np.full(k, H - BORDER - 1 - d))):
            us.append(ru), vs.append(rv), ids.append(rng.uniform(0.12, 0.2, k))
    # far outside the reference image (the reference sample must not read there) and negative
    us.append(np.array([-3.5, W + 40.25, 1e6, 17.5, 20.5, -1e9])), vs.append(np.array([10.5, 20.5, 30.5, -7.25, H + 1000.5, -1e9])), ids.append(np.full(6, 0.15))
    # behind the target camera: t_z of T_target_reference is negative here (the target moved forward), so rho > -P_z(ray) / t_z puts the
    # point behind it; rho stays inside the idepth range
    T_tr = np.linalg.inv(base["T_w_tgt"]) @ base["T_w_ref"]
    Uu, _ = _matrices(base["intr"], base["tgt_intr"], T_tr)
    bu, bv = rng.uniform(30, W - 30, 2 * k), rng.uniform(30, H - 30, 2 * k)
    zray = Uu[2, 0] * bu + Uu[2, 1] * bv + Uu[2, 2]
    assert Uu[2, 3] < 0, "the scene's motion is forward"
    rho0 = -zray / Uu[2, 3]
    us.append(bu), vs.append(bv), ids.append(rho0 * np.concatenate([np.full(k, 1.05), np.full(k, 3.0)]))
    # a body of ordinary points so that the system is well conditioned
    bu, bv, bi = random_points(600, 78)
    us.append(bu), vs.append(bv), ids.append(bi)
    c = _case(np.concatenate(us), np.concatenate(vs), np.concatenate(ids), mask=base["mask"], name="edges", target=tgt)
    return _keep_clear(c, F64_MARGIN, False)


COUNTS = (1, 2, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 10240, 10241, 65536, 65537, 70001)


@functools.lru_cache(maxsize=None)
def _count_pool():
    u, v, idp = random_points(4096, 1000)
    c = _case(u, v, idp)
    ok = first_iteration(c)["lin0"]["valid"]
    return u[ok], v[ok], idp[ok]


@functools.lru_cache(maxsize=None)
def count_case(n):
    """n points drawn with replacement from ~4000 non-integer positions that are valid at the initial state"""
    u, v, idp = _count_pool()
    k = np.random.default_rng(n).integers(0, len(u), n)
    return _case(u[k], v[k], idp[k], name=f"count{n}")


def oracle_solve(c, rounded=False, **options):
    """the CPU oracle's alignment of a case; rounded: every input the float32 path stores in single precision (points, intensities,
    planes) rounded to float32 and back"""
    from dsopp_amd import synthetic as syn
    from oracle import pyoracle as po
    r = (lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)) if rounded else (lambda a: a)
    return po.align_solve(po.default_align_options(**options_kw(c, **options)), r(c["u"]), r(c["v"]), r(c["idepth"]), r(c["intensity"]), c["intr"], c["size"],
                          syn.mat_to_params(c["T_w_ref"]), c["e_ref"], c["ab_ref"], c["tgt_intr"], r(c["tgt_planes"]), c["mask"], syn.mat_to_params(c["T_w_tgt"]),
                          c["e_tgt"], c["ab_tgt"])


F32_FACTOR = 8.0   # bars of the float32 device tests = F32_FACTOR x what single precision does to the same case on the CPU


F32_DRAWS = 8


@functools.lru_cache(maxsize=None)
def f32_first_iteration_sensitivity(name, n):
    """the float32 model against the float64 model on the float32 case (name, n) after one iteration: dict(H: relative to max |H|,
    H_scaled: scaled_rel, energy: relative, pose: absolute on the 7 pose parameters, affine: absolute).  A sum of n rounding errors is a
    random quantity of which ONE evaluation may happen to be small, so each figure is the largest of F32_DRAWS evaluations: the case's
    own start and starts moved by twists of ~1e-6 (1e-4 px: the roundings change, the problem does not)."""
    from dsopp_amd import synthetic as syn
    c = dict(case(name, n, True))
    rng = np.random.default_rng(n)
    T0 = c["T_w_tgt"]
    i32 = reference_intensity(c["ref_planes"], c["u"], c["v"], np.float32)     # the reference sample is taken in single precision as well
    out = dict(H=0.0, H_scaled=0.0, energy=0.0, pose=0.0, affine=0.0)
    for k in range(F32_DRAWS):
        c["T_w_tgt"] = T0 if k == 0 else T0 @ se3_exp(rng.normal(0, 1e-6, 6))
        f64, f32 = first_iteration(c), first_iteration(c, dtype=np.float32, intensity=i32)
        assert f64["n_valid"] == f32["n_valid"] and f64["accepted"] == f32["accepted"]
        got = dict(H=rel(f32["H"], f64["H"]), H_scaled=scaled_rel(f32["H"], f64["H"]), energy=abs(f32["energy"] - f64["energy"]) / abs(f64["energy"]),
                   pose=float(np.abs(syn.mat_to_params(f32["T_w_target"]) - syn.mat_to_params(f64["T_w_target"])).max()),
                   affine=float(np.abs(f32["affine"] - f64["affine"]).max()))
        out = {key: max(out[key], got[key]) for key in out}
    return out


@functools.lru_cache(maxsize=None)
def f32_end_state_sensitivity(name, n):
    """the oracle's full solve on float32-rounded inputs against its solve on the float32 case (name, n) as it is: dict(pose, affine, energy
    (relative), iterations (pair))"""
    c = case(name, n, True)
    a, b = oracle_solve(c), oracle_solve(c, rounded=True)
    return dict(pose=float(np.abs(a["T_w_target"] - b["T_w_target"]).max()), affine=float(np.abs(a["affine_brightness"] - b["affine_brightness"]).max()),
                energy=abs(a["energy"] - b["energy"]) / abs(a["energy"]), iterations=(a["iterations"], b["iterations"]))


def scaled_rel(H, H_ref):
    """max |H - H_ref|_ij / sqrt(H_ref,ii H_ref,jj): the affine prior (1e12 by default) does not hide the pose block as it does in a
    difference relative to max |H|"""
    d = np.sqrt(np.abs(np.diag(H_ref)))
    d[d == 0] = 1.0
    return float((np.abs(np.asarray(H) - H_ref) / np.outer(d, d)).max())


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), np.finfo(np.float64).tiny))
