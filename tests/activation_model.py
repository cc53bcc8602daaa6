"""The NumPy statement of the activation of immature landmarks (reference: src/tracker/landmarks_activator/src/landmarks_activator.cpp:29-391,
ImmatureTrackingLandmark::readyForActivation, ActiveKeyframe::applyImmatureLandmarkActivationStatuses): the per-landmark status, the rules for
the active landmarks, the P-regulator, the sequential greedy selection as the O(n^2) double loop it is in the reference (no grid, no rounds)
and the 3-iteration Levenberg-Marquardt on the inverse depth.  It imports neither the CPU oracle nor the library.
tests/test_activation_model.py pins it on the CPU oracle, tests/test_gpu_activation_edges.py holds the device to it.

Frames are the dicts the oracle's activate_landmarks takes (oldest first, the newest keyframe last): pixelinfo (H x W x 3), mask (H x W u8 or
None), T_w (qx, qy, qz, qw, tx, ty, tz), exposure, affine; all but the last also active_uv, active_idepth, active_flags (bit 1 marginalised,
bit 2 outlier — what set_landmarks takes; absent: active_skip, taken as the outlier bit) and `immature` (the struct of arrays, or None).
Nothing is changed in place.

The selection's coordinate and distance arithmetic takes a scalar type: np.float64 (the arithmetic of the oracle and of the device),
np.longdouble, or fractions.Fraction (exact: squared distances are compared with the squared distance).  The refinement takes np.float64 or
np.longdouble."""
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

ACTIVATE, SKIP, DELETE = 0, 1, 2                                             # ImmatureLandmarkActivationStatus
IMM_GOOD, IMM_OOB, IMM_OUTLIER, IMM_SKIPPED, IMM_ILL, IMM_UNINIT, IMM_DELETE = range(7)   # ImmatureLandmarkStatus as the C-ABI encodes it
FLAG_MARGINALIZED, FLAG_OUTLIER = 1, 2
PATTERN = ((0, 2), (-1, 1), (1, 1), (-2, 0), (0, 0), (2, 0), (-1, -1), (0, -2))
MAX_ENERGY_FOR_INLIERS = 8 * 12 * 12                                         # :130
BORDER = 4                                                                   # camera_model_base.hpp:34

# statuses / states / idepth: one array per keyframe but the newest (states: dict(status, idepth_min, idepth_max) as the call leaves the set, None
# for a keyframe without a set); n_active: number_of_active_points; distance: the regulated distance; records: {(keyframe, index): Branches} of
# every landmark the selection accepted (refine only); n_candidates: landmarks that reached the selection; n_waiting: candidates that no active
# landmark blocks and that have an earlier candidate within the distance (what the device's greedy rounds are left with); max_earlier: the most
# earlier candidates any candidate has within the distance
Result = namedtuple("Result", "statuses n_active distance states idepth records n_candidates n_waiting max_earlier")
# accepted / rejected: LM steps; rejected_then_iterated: a rejected step was followed by another iteration (on the kept linearisation);
# no_valid_at_start: n_valid was 0 before the first iteration; huber / over_cutoff: some target of some evaluation was Huber-weighted / at or
# over the inlier cut-off
Branches = namedtuple("Branches", "accepted rejected rejected_then_iterated converged no_valid_at_start zero_hessian huber over_cutoff")


def _scalar(S):
    """x (a binary64 number) -> S, exactly"""
    if S is Fraction:
        return lambda x: Fraction(float(x))
    return lambda x: S(x)


# ---- rigid transforms and the reprojection matrices (camera_reproject.hpp:250-258), over any scalar type
def _rigid(params, c):
    x, y, z, w = (c(v) for v in params[:4])
    one, two = c(1.0), c(2.0)
    R = [[one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w)],
         [two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w)],
         [two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)]]
    return R, [c(v) for v in params[4:7]]


def _inverse(T):
    R, t = T
    Rt = [[R[j][i] for j in range(3)] for i in range(3)]
    return Rt, [-(Rt[i][0] * t[0] + Rt[i][1] * t[1] + Rt[i][2] * t[2]) for i in range(3)]


def _mul(A, B):
    (Ra, ta), (Rb, tb) = A, B
    R = [[Ra[i][0] * Rb[0][j] + Ra[i][1] * Rb[1][j] + Ra[i][2] * Rb[2][j] for j in range(3)] for i in range(3)]
    return R, [Ra[i][0] * tb[0] + Ra[i][1] * tb[1] + Ra[i][2] * tb[2] + ta[i] for i in range(3)]


def _reprojectors(T, fx, fy, cx, cy, one):
    """-> (K [R|t] K^-1, [R|t] K^-1), 12 numbers each, row-major 3 x 4"""
    R, t = T
    ifx, ify, k02, k12 = one / fx, one / fy, -cx / fx, -cy / fy
    U = []
    for i in range(3):
        U += [R[i][0] * ifx, R[i][1] * ify, R[i][0] * k02 + R[i][1] * k12 + R[i][2], t[i]]
    M = [fx * U[j] + cx * U[8 + j] for j in range(4)] + [fy * U[4 + j] + cy * U[8 + j] for j in range(4)] + U[8:12]
    return M, U


def valid_idepth(idepth):
    return idepth > -1e-4 and idepth < 1.0 / 0.001 + 1e1                     # camera_model_base.hpp:67-74


def _inside_roi(u, v, W, H):
    return u >= BORDER and v >= BORDER and u <= W - BORDER - 1 and v <= H - BORDER - 1   # camera_model_base.hpp:52-60


def _round_half_up(x):
    return math.floor(x + Fraction(1, 2)) if isinstance(x, Fraction) else int(np.floor(x + 0.5))


def mask_valid(mask, W, H, x, y):
    """CameraMask::valid of a point: the ROUNDED position (std::round: halves away from zero; here floor(x + 0.5) — NumPy's round is half to
    even — and every caller has the point inside the camera ROI, so no negative half arises), border-checked; mask None = all valid"""
    mx, my = _round_half_up(x), _round_half_up(y)
    if mx < 0 or mx >= W or my < 0 or my >= H:
        return False
    return True if mask is None else bool(mask[my, mx] != 0)


def _reproject(M, u, v, idepth, rho_valid, W, H):
    """ArrayReprojector<.., true>::reproject of one point (camera_reproject.hpp:270-293) -> (tu, tv) or None"""
    ok = rho_valid and _inside_roi(u, v, W, H)
    x = M[0] * u + M[1] * v + (M[2] + M[3] * idepth)
    y = M[4] * u + M[5] * v + (M[6] + M[7] * idepth)
    z = M[8] * u + M[9] * v + (M[10] + M[11] * idepth)
    if not (ok and z > 0):
        return None
    tu, tv = x / z, y / z
    return (tu, tv) if _inside_roi(tu, tv, W, H) else None


# ---- the rules
def active_rules(idepth, flags):
    """what updateFrame hands to the keyframe (photometric_bundle_adjustment.cpp:233-239) and reprojectActivePoints makes of it (:65):
    |idepth| < 1e-8 is flushed to 0, a negative inverse depth is an outlier; -> (idepth, counted)"""
    outlier = bool(flags & FLAG_OUTLIER)
    idepth = float(idepth)
    if abs(idepth) < 1e-8:
        idepth = 0.0
    elif idepth < 0:
        outlier = True
    return idepth, not outlier and not (flags & FLAG_MARGINALIZED)


def active_flags(frame):
    if frame.get("active_flags") is not None:
        return np.asarray(frame["active_flags"], dtype=np.uint8)
    return (np.asarray(frame["active_skip"], dtype=np.uint8) != 0).astype(np.uint8) * FLAG_OUTLIER


def ready_for_activation(status, search_pixel_interval, uniqueness, idepth):
    """ImmatureTrackingLandmark::readyForActivation — immature_tracking_landmark.cpp:46-52"""
    return status in (IMM_GOOD, IMM_OOB, IMM_SKIPPED, IMM_ILL) and search_pixel_interval < 8 and uniqueness > 3 and idepth > 0


def regulate(distance, n_active, desired):
    """recalculateMinDistanceToNeighbor — :29-39"""
    d = float(distance) + (float(n_active) - float(desired)) * 0.001
    return min(max(d, 0.0), 10.0)


def select(active_points, candidates, distance, S=np.float64):
    """haveNoNeighbors over the growing list of reprojected points (:41-49, :107-110): candidates in order, accepted when no reprojected active
    landmark and no earlier ACCEPTED candidate is closer than the distance (strictly).  -> (accepted flags, n_waiting, max_earlier)"""
    exact = S is Fraction
    if S is np.float64:   # (Python's float is binary64 with the same correctly rounded *, +, sqrt)
        active_points = [(float(x), float(y)) for x, y in active_points]
        candidates = [(float(x), float(y)) for x, y in candidates]
        d, root = float(distance), math.sqrt
    else:
        d, root = _scalar(S)(distance), np.sqrt
    dd = d * d

    def within(p, q):
        dx, dy = q[0] - p[0], q[1] - p[1]
        return dx * dx + dy * dy < dd if exact else root(dx * dx + dy * dy) < d

    accepted, n_waiting, max_earlier = [], 0, 0
    for g, p in enumerate(candidates):
        by_active = any(within(p, q) for q in active_points)
        earlier = [j for j in range(g) if within(p, candidates[j])]
        accepted.append(not by_active and not any(accepted[j] for j in earlier))
        n_waiting += (not by_active) and len(earlier) > 0
        max_earlier = max(max_earlier, len(earlier))
    return accepted, n_waiting, max_earlier


# ---- the refinement (LandmarkActivationProblem :128-277, optimizeImmatureLandmark :279-311)
class _Refiner:
    def __init__(self, frames, intrinsics, sigma, D):
        self.D, self.F = D, len(frames)
        self.H, self.W = frames[0]["pixelinfo"].shape[:2]
        self.pix = [np.asarray(f["pixelinfo"], dtype=np.float64) for f in frames]
        self.masks = [f.get("mask") for f in frames]
        self.T = [_rigid(f["T_w"], D) for f in frames]
        self.expo = [D(f.get("exposure", 1.0)) for f in frames]
        self.aff = [(D(f.get("affine", (0, 0))[0]), D(f.get("affine", (0, 0))[1])) for f in frames]
        self.intr = [D(v) for v in intrinsics]
        self.sigma = D(sigma)
        self.px = np.array([p[0] for p in PATTERN], dtype=D)
        self.py = np.array([p[1] for p in PATTERN], dtype=D)
        self._pairs = {}

    def pair(self, r, t):
        if (r, t) not in self._pairs:
            D = self.D
            Ttr = _mul(_inverse(self.T[t]), self.T[r])                       # :169
            M, U = _reprojectors(Ttr, *self.intr, D(1.0))
            scale = (self.expo[t] / self.expo[r]) * np.exp(self.aff[t][0] - self.aff[r][0])   # :166-167
            self._pairs[(r, t)] = (M, U, Ttr[1], scale, self.aff[t][1], self.aff[r][1])
        return self._pairs[(r, t)]

    def _valid(self, t, idepth, ref_inside, z, tu, tv):
        W, H = self.W, self.H
        if not (valid_idepth(idepth) and ref_inside and bool(np.all(z > 0))):
            return False
        if not bool(np.all((tu >= BORDER) & (tv >= BORDER) & (tu <= W - BORDER - 1) & (tv <= H - BORDER - 1))):
            return False
        return all(mask_valid(self.masks[t], W, H, x, y) for x, y in zip(tu, tv))

    def _sample(self, t, tu, tv, channels):
        """interpolateLinear — pixel_map.hpp:20-40"""
        D = self.D
        ix, iy = tu.astype(np.int64), tv.astype(np.int64)
        dx, dy = tu - ix.astype(D), tv - iy.astype(D)
        dxdy = dx * dy
        p = self.pix[t]
        w11, w01, w10, w00 = dxdy, dy - dxdy, dx - dxdy, 1 - dx - dy + dxdy
        return [w11 * p[iy + 1, ix + 1, c].astype(D) + w01 * p[iy + 1, ix, c].astype(D) + w10 * p[iy, ix + 1, c].astype(D) + w00 * p[iy, ix, c].astype(D)
                for c in range(channels)]

    def _sum(self, values):
        s = self.D(0)
        for v in values:
            s = s + v
        return s

    def refine(self, r, projection, patch, idepth0, minimum_inliers):
        """-> (status, idepth, Branches)"""
        D, F, sigma = self.D, self.F, self.sigma
        ru, rv = D(projection[0]) + self.px, D(projection[1]) + self.py        # PatternPatch::shiftPattern
        patch = np.asarray(patch, dtype=np.float64).astype(D)
        W, H = self.W, self.H
        ref_inside = bool(np.all((ru >= BORDER) & (rv >= BORDER) & (ru <= W - BORDER - 1) & (rv <= H - BORDER - 1)))
        st = dict(idepth=D(idepth0), stop=False, hessian=D(0), b=D(0), huber=False, over=False, zero_hessian=False)

        def calculate_energy():                                               # :150-202
            energy, n_valid = D(0), 0
            if st["stop"]:
                st["idepth"] = D(-1)
                return energy, n_valid
            idepth = st["idepth"]
            for t in range(F):
                if t == r:
                    continue
                M, _, _, scale, b_t, b_r = self.pair(r, t)
                x = M[0] * ru + M[1] * rv + (M[2] + M[3] * idepth)
                y = M[4] * ru + M[5] * rv + (M[6] + M[7] * idepth)
                z = M[8] * ru + M[9] * rv + (M[10] + M[11] * idepth)
                tu, tv = x / z, y / z
                if not self._valid(t, idepth, ref_inside, z, tu, tv):
                    continue
                rr = (self._sample(t, tu, tv, 1)[0] - b_t) - scale * (patch - b_r)
                sq = self._sum(rr * rr)
                norm = np.sqrt(sq)
                if norm > sigma:
                    st["huber"] = True
                hw = sigma / norm if norm > sigma else D(1)
                if sq < MAX_ENERGY_FOR_INLIERS:
                    energy = energy + hw * sq
                    n_valid += 1
                else:
                    energy = energy + D(MAX_ENERGY_FOR_INLIERS)
                    st["over"] = True
            if n_valid == 0:
                st["idepth"] = D(-1)
                st["stop"] = True
            return energy, n_valid

        def linearize():                                                      # :204-256
            hessian, b = D(0), D(0)
            idepth = st["idepth"]
            fx, fy, cx, cy = self.intr
            for t in range(F):
                if t == r:
                    continue
                _, U, tr, scale, b_t, b_r = self.pair(r, t)
                X = U[0] * ru + U[1] * rv + (U[2] + U[3] * idepth)            # camera_reproject.hpp:305-367
                Y = U[4] * ru + U[5] * rv + (U[6] + U[7] * idepth)
                Z = U[8] * ru + U[9] * rv + (U[10] + U[11] * idepth)
                tu, tv = (fx * X + cx * Z) / Z, (fy * Y + cy * Z) / Z
                rescaling = 1 / Z
                b0, b1 = X * rescaling, Y * rescaling
                dui = fx * (tr[0] * rescaling - tr[2] * (rescaling * b0))
                dvi = fy * (tr[1] * rescaling - tr[2] * (rescaling * b1))
                if not self._valid(t, idepth, ref_inside, Z, tu, tv):
                    continue
                sI, sIx, sIy = self._sample(t, tu, tv, 3)
                rr = (sI - b_t) - scale * (patch - b_r)
                norm = np.sqrt(self._sum(rr * rr))
                if norm > sigma:
                    st["huber"] = True
                hw = sigma / norm if norm > sigma else D(1)
                d = sIx * dui + sIy * dvi
                hessian = hessian + self._sum((hw * d) * d)
                b = b + self._sum((hw * d) * rr)
            st["hessian"], st["b"] = hessian, b
            if hessian == 0:
                st["stop"] = True
                st["zero_hessian"] = True

        # levenberg_marquardt_algorithm::solve (levenberg_marquardt_algorithm.hpp:77-128) with the options of :286-292: at most 3 iterations,
        # lambda 0.1, / 2 on accept, x 5 on reject, function tolerance 0 (never reached), parameter tolerance 1e-8
        with np.errstate(all="ignore"):
            lam = D(1) / D(10)
            result_energy, result_valid = calculate_energy()
            no_valid_at_start = result_valid == 0
            accepted = rejected = 0
            rejected_then_iterated = converged = system_valid = last_rejected = False
            for _ in range(3):
                if converged or result_valid <= 0:
                    break
                if last_rejected:
                    rejected_then_iterated = True
                if not system_valid:
                    linearize()
                step = st["b"] / (st["hessian"] + st["hessian"] * lam)         # calculateStep :258-262
                old = st["idepth"]
                st["idepth"] = old - step
                next_energy, n_valid = calculate_energy()
                if n_valid == 0:
                    st["idepth"] = old                                         # rejectStep
                    break
                if next_energy < result_energy:
                    converged = converged or bool(step * step < D(1e-8) * (st["idepth"] * st["idepth"] + D(1e-8)))   # acceptStep :264
                    result_energy, result_valid = next_energy, n_valid
                    lam = lam / 2
                    system_valid = last_rejected = False
                    accepted += 1
                else:
                    st["idepth"] = old
                    lam = lam * 5
                    system_valid = last_rejected = True
                    rejected += 1
            calculate_energy()                                                # :126: its side effect on the inverse depth is what matters
        rec = Branches(accepted, rejected, rejected_then_iterated, converged, no_valid_at_start, st["zero_hessian"], st["huber"], st["over"])
        if result_valid < minimum_inliers or st["idepth"] < 0:                # :305-306
            return DELETE, None, rec
        return ACTIVATE, st["idepth"], rec


# ---- the call
def activate(frames, intrinsics, sigma_huber_loss=20.0, number_of_desired_points=2000, min_distance_to_neighbor=0.0, refine=True,
             mask_sparsity_newest=None, scalar=np.float64, refine_dtype=np.float64):
    """LandmarksActivator::activate (:351-391) followed by applyImmatureLandmarkActivationStatuses (active_keyframe.cpp:232-235)"""
    S, c = scalar, _scalar(scalar)
    H, W = frames[0]["pixelinfo"].shape[:2]
    sw, sh = W // 2, H // 2                                                   # the mask image of the sparsity level (pyramid level 1)
    swd, shd = c(W) / c(2.0), c(H) / c(2.0)                                   # its camera model's size: may be fractional
    fx, fy, cx, cy = (c(v) / c(2.0) for v in intrinsics)
    T_newest_inv = _inverse(_rigid(frames[-1]["T_w"], c))
    Ms = [_reprojectors(_mul(T_newest_inv, _rigid(f["T_w"], c)), fx, fy, cx, cy, c(1.0))[0] for f in frames[:-1]]
    two = c(2.0)
    # reprojectActivePoints :51-87
    n_active, active_points = 0, []
    for f, M in zip(frames[:-1], Ms):
        for uv, rho, flg in zip(np.asarray(f["active_uv"]).reshape(-1, 2), f["active_idepth"], active_flags(f)):
            rho, counted = active_rules(rho, int(flg))
            if not counted:
                continue
            n_active += 1
            q = _reproject(M, c(uv[0]) / two, c(uv[1]) / two, c(rho), valid_idepth(rho), swd, shd)
            if q is not None and mask_valid(mask_sparsity_newest, sw, sh, *q):
                active_points.append(q)
    distance = regulate(min_distance_to_neighbor, n_active, number_of_desired_points)
    # activationStatus :89-126, the part of one landmark
    statuses, idepths, candidates, where = [], [], [], []
    for k, (f, M) in enumerate(zip(frames[:-1], Ms)):
        l = f.get("immature")
        n = 0 if l is None else len(l["status"])
        st = np.zeros(n, dtype=np.uint8)
        mid = np.zeros(n)
        for i in range(n):
            s = int(l["status"][i])
            mid[i] = float(l["idepth_max"][i]) * 0.5 + float(l["idepth_min"][i]) * 0.5   # ImmatureTrackingLandmark::idepth()
            if s == IMM_DELETE or not l["traced"][i] or s == IMM_OUTLIER:
                st[i] = DELETE
            elif not ready_for_activation(s, l["search_pixel_interval"][i], l["uniqueness"][i], mid[i]):
                st[i] = DELETE if s == IMM_OOB else SKIP
            else:
                q = _reproject(M, c(l["projection"][i][0]) / two, c(l["projection"][i][1]) / two, c(mid[i]), valid_idepth(mid[i]), swd, shd)
                if q is None or not mask_valid(mask_sparsity_newest, sw, sh, *q):
                    st[i] = DELETE
                else:
                    st[i] = SKIP                                              # until the selection accepts it
                    candidates.append(q)
                    where.append((k, i))
        statuses.append(st)
        idepths.append(mid)
    accepted, n_waiting, max_earlier = select(active_points, candidates, distance, S)
    for (k, i), a in zip(where, accepted):
        if a:
            statuses[k][i] = ACTIVATE
    # optimizeImmatureLandmarks :313-338
    states, records = [], {}
    for f in frames[:-1]:
        l = f.get("immature")
        states.append(None if l is None else dict(status=np.array(l["status"], dtype=np.uint8), idepth_min=np.array(l["idepth_min"], dtype=np.float64),
                                                  idepth_max=np.array(l["idepth_max"], dtype=np.float64)))
    if refine:
        ref = _Refiner(frames, intrinsics, sigma_huber_loss, refine_dtype)
        minimum_inliers = min(1, len(frames) - 1)
        for (k, i), a in zip(where, accepted):
            if not a:
                continue
            l = frames[k]["immature"]
            status, idepth, rec = ref.refine(k, l["projection"][i], l["patch"][i], idepths[k][i], minimum_inliers)
            records[(k, i)] = rec
            statuses[k][i] = status
            if status == ACTIVATE:
                states[k]["idepth_min"][i] = states[k]["idepth_max"][i] = idepths[k][i] = float(idepth)
    for st, state in zip(statuses, states):                                   # activated and deleted landmarks are dead afterwards
        if state is not None:
            state["status"][st != SKIP] = IMM_DELETE
    return Result(statuses, n_active, distance, states, idepths, records, len(candidates), n_waiting, max_earlier)
