"""NumPy statement of the reference depth maps and of the optical-flow measure taken from them — the chain the device runs in
depth_map_kernels.hpp (splat -> 2 x 2 pools -> dilation), the row scan of align.hip that turns a level into reference points, and the flow
over those points — vectorised, with the geometry in np.longdouble.  Written from the definitions (createReferenceDepthMaps,
create_depth_maps.cpp:18-147; LocalFrame's depth-map constructor, local_frame.hpp:367-392; calculateMeanSquareOpticalFlow,
monocular_tracker.cpp:104-134), not from the kernels; pinned by tests/test_depth_maps_model.py against the CPU oracle and against the loop
statement of tests/test_depth_maps.py.

The module also holds the case table CASES that the CPU tests and tests/test_gpu_depth_map_edges.py share.  Two families:
  exact    fx = fy = 256, dyadic principal point, identity rotations, dyadic translations (t_z = 0 wherever a landmark is meant to land),
           integer or dyadic uv, dyadic idepth: every product and sum of the projection is exact in double, so a landmark ON a ROI border
           or ON a rounding tie is decided identically by every correct implementation, fused multiply-adds or not.  splat() reports
           `exact` (the float64 evaluation of every decision quantity is bit-equal to the longdouble one): a condition of these cases.
  general  seeded random motions of the size synthetic.BASE_MOTION produces, integer uv.  splat() counts the AMBIGUOUS landmarks, those
           whose projection lies within 1e-9 px of a ROI border or of a rounding tie (or whose z lies within 1e-12 of 0) — a correct
           implementation may decide those either way.  The seeds are chosen so that the count is 0: a condition, not a tolerance."""
import collections
import functools

import numpy as np

LD = np.longdouble
BORDER = 4                    # CameraModelBase::insideCameraROI: [4, W - 5] x [4, H - 5]
MIN_POINT_IDEPTH = 1e-6       # LocalFrame depth-map constructor / calculateMeanSquareOpticalFlow
CONSTANT_VARIANCE = 1e-5      # estimate_uncertainty off (photometric_bundle_adjustment.cpp:254)
AMBIGUOUS_PX, AMBIGUOUS_Z = 1e-9, 1e-12

Splat = collections.namedtuple("Splat", "ids wgt k ambiguous exact")


# ---- geometry ----------------------------------------------------------------------------------------------------------------------------
def _rigid(p, dt):
    """(qx, qy, qz, qw, tx, ty, tz) -> (R, t) in the scalar type dt"""
    x, y, z, w = (dt(v) for v in np.asarray(p, dtype=np.float64)[:4])
    one, two = dt(1), dt(2)
    R = np.array([[one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w)],
                  [two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w)],
                  [two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)]], dtype=dt)
    return R, np.asarray(p, dtype=np.float64)[4:7].astype(dt)


def _relative(T_w_newest, T_w_source, dt):
    """T_newest^-1 T_source"""
    Rn, tn = _rigid(T_w_newest, dt)
    Rs, ts = _rigid(T_w_source, dt)
    return Rn.T @ Rs, Rn.T @ ts - Rn.T @ tn


def _as_rigid(T, dt):
    T = np.asarray(T, dtype=np.float64)
    if T.shape == (4, 4):
        return T[:3, :3].astype(dt), T[:3, 3].astype(dt)
    return _rigid(T, dt)


def _reproject(R, t, intr, u, v, rho, dt):
    """unproject (z = 1) -> transform (point / depth) -> project: x, y, z, tu, tv"""
    fx, fy, cx, cy = (dt(c) for c in intr)
    u, v, rho = u.astype(dt), v.astype(dt), rho.astype(dt)
    dx, dy = (u - cx) / fx, (v - cy) / fy
    with np.errstate(all="ignore"):
        x = R[0, 0] * dx + R[0, 1] * dy + R[0, 2] + rho * t[0]
        y = R[1, 0] * dx + R[1, 1] * dy + R[1, 2] + rho * t[1]
        z = R[2, 0] * dx + R[2, 1] * dy + R[2, 2] + rho * t[2]
        tu, tv = fx * (x / z) + cx, fy * (y / z) + cy
    return x, y, z, tu, tv


def _inside(u, v, W, H):
    with np.errstate(invalid="ignore"):
        return (u >= BORDER) & (v >= BORDER) & (u <= W - 1 - BORDER) & (v <= H - 1 - BORDER)


def _valid_idepth(rho):
    with np.errstate(invalid="ignore"):
        return (rho > -1e-4) & (rho < 1 / 0.001 + 10)


def _same(a64, b):
    a = a64.astype(LD)
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def weights(variance):
    """sqrt(kVariationScale / (variance + kEps)), in double as every implementation computes it (two correctly rounded operations)"""
    return np.sqrt(1e-3 / (np.asarray(variance, dtype=np.float64) + 1e-12))


# ---- the chain ---------------------------------------------------------------------------------------------------------------------------
def splat(sources, T_w_newest, intr, W, H):
    """fillFineDepthMap.  sources: dicts with T_w (7), uv (n x 2), idepth, flags, status, variance (n, or a scalar).
    -> Splat(idepth sums, weights (both H x W float64), hit count per cell, number of ambiguous landmarks, exact)"""
    ids, wgt = np.zeros(H * W, dtype=LD), np.zeros(H * W, dtype=LD)
    k = np.zeros(H * W, dtype=np.int64)
    ambiguous, exact = 0, True
    for s in sources:
        n = len(s["idepth"])
        if n == 0:
            continue
        uv = np.asarray(s["uv"], dtype=np.float64).reshape(n, 2)
        rho = np.asarray(s["idepth"], dtype=np.float64).copy()
        flags, status = np.asarray(s["flags"], dtype=np.uint8), np.asarray(s["status"], dtype=np.uint8)
        with np.errstate(invalid="ignore"):
            rho[np.abs(rho) < 1e-8] = 0                                   # what updateFrame hands to the keyframe ...
            reach = (status == 0) & ((flags & 3) == 0) & ~(rho < 0)       # ... and a negative idepth makes the landmark an outlier
        reach &= _valid_idepth(rho) & _inside(uv[:, 0], uv[:, 1], W, H)
        safe = np.where(np.isfinite(rho), rho, 0.0)                       # (a landmark that is not a number never reaches the projection)
        q = _reproject(*_relative(T_w_newest, s["T_w"], LD), intr, uv[:, 0], uv[:, 1], safe, LD)
        q64 = _reproject(*_relative(T_w_newest, s["T_w"], np.float64), intr, uv[:, 0], uv[:, 1], safe, np.float64)
        exact = exact and all(_same(a, b) for a, b in zip(q64, q))
        _, _, z, tu, tv = q
        with np.errstate(invalid="ignore"):
            front = z > 0
            inside = _inside(tu, tv, W, H)
            near_zero = np.abs(z) <= AMBIGUOUS_Z
            near_border = np.zeros(n, dtype=bool)
            near_tie = np.zeros(n, dtype=bool)
            for t, hi in ((tu, W - 1 - BORDER), (tv, H - 1 - BORDER)):
                near_border |= (np.abs(t - BORDER) <= AMBIGUOUS_PX) | (np.abs(t - hi) <= AMBIGUOUS_PX)
                near_tie |= np.abs(t - np.floor(t) - LD(0.5)) <= AMBIGUOUS_PX
        ambiguous += int(np.sum(reach & (near_zero | (front & (near_border | (inside & near_tie))))))
        keep = reach & front & inside
        if not keep.any():
            continue
        w = weights(np.broadcast_to(np.asarray(s["variance"], dtype=np.float64), (n,)))[keep]
        cell = (np.floor(tv[keep] + LD(0.5)).astype(np.int64)) * W + np.floor(tu[keep] + LD(0.5)).astype(np.int64)
        np.add.at(ids, cell, rho[keep].astype(LD) / z[keep] * w.astype(LD))      # idepth in the newest frame = idepth / depth scale
        np.add.at(wgt, cell, w.astype(LD))
        np.add.at(k, cell, 1)
    return Splat(ids.astype(np.float64).reshape(H, W), wgt.astype(np.float64).reshape(H, W), k.reshape(H, W), ambiguous, exact)


def pool(ids, wgt, levels):
    """fillCoarseDepthMaps: [(ids, wgt)] of `levels` undilated levels; sizes halve with floor, children summed as a, a + 1, b, b + 1"""
    out = [(ids, wgt)]
    for _ in range(1, levels):
        h2, w2 = out[-1][0].shape[0] // 2, out[-1][0].shape[1] // 2
        out.append(tuple(((m[0:2 * h2:2, 0:2 * w2:2] + m[0:2 * h2:2, 1:2 * w2:2]) + m[1:2 * h2:2, 0:2 * w2:2]) + m[1:2 * h2:2, 1:2 * w2:2]
                         for m in out[-1]))
    return out


AXIS = ((1, 0), (-1, 0), (0, 1), (0, -1))      # (dx, dy) in the reference's order, levels > 1
DIAGONAL = ((1, 1), (-1, -1), (1, -1), (-1, 1))  # levels 0 and 1


def dilate_level(ids, wgt, level):
    """dilateDepthMaps of one level: an interior cell without weight takes the mean of its weighted neighbours, read from the undilated planes"""
    H, W = ids.shape
    out_i, out_w = ids.copy(), wgt.copy()
    if H < 3 or W < 3:
        return out_i, out_w
    si, sw, cnt = np.zeros((H - 2, W - 2)), np.zeros((H - 2, W - 2)), np.zeros((H - 2, W - 2))
    for ox, oy in (AXIS if level > 1 else DIAGONAL):
        ni, nw = ids[1 + oy:H - 1 + oy, 1 + ox:W - 1 + ox], wgt[1 + oy:H - 1 + oy, 1 + ox:W - 1 + ox]
        has = nw > 0
        si = si + np.where(has, ni, 0.0)
        sw = sw + np.where(has, nw, 0.0)
        cnt = cnt + has
    fill = ~(wgt[1:-1, 1:-1] > 0) & (cnt > 0)
    safe = np.where(cnt > 0, cnt, 1.0)
    out_i[1:-1, 1:-1] = np.where(fill, si / safe, ids[1:-1, 1:-1])
    out_w[1:-1, 1:-1] = np.where(fill, sw / safe, wgt[1:-1, 1:-1])
    return out_i, out_w


def dilate(maps):
    return [dilate_level(a, b, lvl) for lvl, (a, b) in enumerate(maps)]


def depth_maps(sources, T_w_newest, intr, W, H, levels):
    """createReferenceDepthMaps: ([(ids, wgt)] per level, the Splat of level 0)"""
    s = splat(sources, T_w_newest, intr, W, H)
    return dilate(pool(s.ids, s.wgt, levels)), s


def level_sizes(W, H, levels):
    return [(W >> l, H >> l) for l in range(levels)]


def reference_points(ids, wgt):
    """the level's reference points, row-major: n x 3 of (x, y, idepth)"""
    H, W = ids.shape
    m = np.zeros((H, W), dtype=bool)
    m[BORDER:H - BORDER, BORDER:W - BORDER] = True
    m &= wgt > 0
    rho = ids / np.where(wgt > 0, wgt, 1.0)
    m &= ~(rho < MIN_POINT_IDEPTH)
    ys, xs = np.nonzero(m)
    return np.stack([xs.astype(np.float64), ys.astype(np.float64), rho[m]], axis=1)


def flow(ids, wgt, intr, T):
    """calculateMeanSquareOpticalFlow of one level under T_target_reference (4 x 4 or 7-vector): (rms bearing distance, pixel count);
    NaN for a level without such a pixel, as 0 / 0 gives in the reference"""
    H, W = ids.shape
    pts = reference_points(ids, wgt)
    fx, fy, cx, cy = (LD(c) for c in intr)
    R, t = _as_rigid(T, LD)
    x, y, z, tu, tv = _reproject(R, t, intr, pts[:, 0], pts[:, 1], pts[:, 2], LD)
    with np.errstate(invalid="ignore"):
        ok = _valid_idepth(pts[:, 2]) & _inside(pts[:, 0], pts[:, 1], W, H) & (z > 0) & _inside(tu, tv, W, H)
    n = int(ok.sum())
    if n == 0:
        return float("nan"), 0
    ax, ay = (pts[ok, 0].astype(LD) - cx) / fx, (pts[ok, 1].astype(LD) - cy) / fy
    bx, by = x[ok] / z[ok], y[ok] / z[ok]
    return float(np.sqrt(np.sum((ax - bx) ** 2 + (ay - by) ** 2) / LD(n))), n


def same_or_both_nan(a, b, tol):
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= tol


# ---- what the other statements take ------------------------------------------------------------------------------------------------------
def oracle_sources(sources):
    """the same landmarks as oracle.pyoracle.create_reference_depth_maps and the loop statement of tests/test_depth_maps.py take them:
    |idepth| < 1e-8 clamped and negative ones skipped beforehand (both leave that to their caller, as the reference leaves it to updateFrame);
    a source without landmarks is left out"""
    out = []
    for s in sources:
        n = len(s["idepth"])
        if n == 0:
            continue
        rho = np.asarray(s["idepth"], dtype=np.float64).copy()
        with np.errstate(invalid="ignore"):
            rho[np.abs(rho) < 1e-8] = 0
            skip = ((np.asarray(s["flags"], dtype=np.uint8) & 3) != 0) | (rho < 0)
        out.append(dict(T_w=np.asarray(s["T_w"], dtype=np.float64), uv=np.asarray(s["uv"], dtype=np.float64).reshape(n, 2), idepth=rho,
                        variance=np.broadcast_to(np.asarray(s["variance"], dtype=np.float64), (n,)).copy(), skip=skip.astype(np.uint8),
                        status=np.asarray(s["status"], dtype=np.uint8)))
    return out


def model_sources(case, variances=None, flags=None, poses=None, idepths=None, statuses=None):
    """the case's landmarks as splat() takes them; `variances` etc.: per-source arrays read back from a window, replacing the case's own"""
    poses = case["poses"] if poses is None else poses
    out = []
    for i, s in enumerate(case["sources"]):
        out.append(dict(T_w=poses[i], uv=s["uv"], idepth=s["idepth"] if idepths is None else idepths[i],
                        flags=s["flags"] if flags is None else flags[i], status=s["status"] if statuses is None else statuses[i],
                        variance=CONSTANT_VARIANCE if variances is None else variances[i]))
    return out


def case_maps(case, **kw):
    """(dilated levels, Splat) of a case with constant variances (or with what `kw` reads back, see model_sources)"""
    poses = kw.get("poses") or case["poses"]
    return depth_maps(model_sources(case, **kw), poses[-1], case["intr"], case["W"], case["H"], case["levels"])


def flow_transforms():
    """the four relative poses of tests/test_depth_maps.py: _flow_case — general, translation only, identity, large"""
    from dsopp_amd import synthetic as syn
    return [syn.se3_exp(np.array([0.05, -0.02, 0.03, 0.01, -0.02, 0.005])), syn.se3_exp(np.array([0.05, -0.02, 0.03, 0, 0, 0])),
            np.eye(4), syn.se3_exp(np.array([0.3, 0.1, -0.2, 0.05, 0.08, -0.03]))]


# ---- the case table ----------------------------------------------------------------------------------------------------------------------
IDENTITY = np.array([0, 0, 0, 1.0, 0, 0, 0])
SPECIAL_IDEPTHS = (0.0, 5e-9, -5e-9, -1e-8, -1e-3, 1009.0, 1010.5, np.nan, np.inf, -np.inf)
SPECIAL_KEPT = (1, 1, 1, 0, 0, 1, 0, 0, 0, 0)     # clamped to 0 and kept | negative: outlier | validIdepth | not a number


def _pose(t):
    return np.concatenate([IDENTITY[:4], np.asarray(t, dtype=np.float64)])


def _source(uv, idepth, flags=None, status=None):
    n = len(idepth)
    return dict(uv=np.asarray(uv, dtype=np.float64).reshape(n, 2), idepth=np.asarray(idepth, dtype=np.float64),
                flags=np.zeros(n, dtype=np.uint8) if flags is None else np.asarray(flags, dtype=np.uint8),
                status=np.zeros(n, dtype=np.uint8) if status is None else np.asarray(status, dtype=np.uint8))


def _exact_intr(W, H):
    return np.array([256.0, 256.0, W / 2.0, H / 2.0])


def _roi_cells(W, H):
    ys, xs = np.mgrid[BORDER:H - BORDER, BORDER:W - BORDER]
    return np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.float64)


def _dyadic_idepth(n, rng):
    return rng.integers(1, 33, n) / 16.0          # 1/16 .. 2


def _edges():
    """77 x 59 x 5, exact: every decision edge of the splat at once.  `expect`: the designed hit count of every cell that is hit"""
    W, H = 77, 59
    e = 2.0 ** -20
    expect = {}

    def hit(x, y, k=1):
        expect[(x, y)] = expect.get((x, y), 0) + k

    # source 0: no motion — a landmark lands on its own pixel, whatever its idepth
    uv, rho, flg, st = [], [], [], []

    def add0(u, v, r=1.0, f=0, s=0, kept=1):
        uv.append((u, v)), rho.append(r), flg.append(f), st.append(s)
        if kept:
            hit(int(u), int(v))
    for u, v in ((4, 4), (W - 5, 4), (4, H - 5), (W - 5, H - 5)):       # ON the border: kept
        add0(u, v)
    for u, v in ((4 - e, 10), (W - 5 + e, 10), (10, 4 - e), (10, H - 5 + e)):   # 2^-20 outside the SOURCE ROI: dropped
        add0(u, v, kept=0)
    for j, (r, kept) in enumerate(zip(SPECIAL_IDEPTHS, SPECIAL_KEPT)):  # idepth edges, one pixel each, three pixels apart
        add0(8 + 3 * j, 8, r=r, kept=kept)
    for j, f in enumerate((0, 1, 2, 3, 4, 8)):                           # only marginalised / outlier skip
        add0(8 + 3 * j, 14, f=f, kept=0 if f & 3 else 1)
    for j, s in enumerate((0, 1, 2, 3)):                                 # only connection status OK counts
        add0(8 + 3 * j, 20, s=s, kept=1 if s == 0 else 0)
    for j in range(30):                                                  # 30 of the 64 landmarks stacked on (40, 30)
        add0(40, 30, r=(j + 1) / 16.0)
    add0(50, 40, r=0.75)                                                 # one of the 2 on (50, 40)
    add0(20, 45, r=0.5)                                                  # the isolated cell (nothing within 4 cells of it)
    s0 = _source(uv, rho, flg, st)
    # source 1: t = (2^-9, 2^-10, 0): a landmark moves by (idepth / 2, idepth / 4) px
    uv1 = [(10, 10.75), (15, 15)] + [(39.75 + j / 128.0, 29.75) for j in range(20)]
    rho1 = [1.0, 2.0] + [1.0] * 20
    hit(11, 11), hit(16, 16), hit(40, 30, 20)                            # x tie 10.5 -> 11; y tie 15.5 -> 16 (both round up); 20 more on (40, 30)
    s1 = _source(uv1, rho1)
    # source 2: t = (-2^-28, -2^-28, 0): moves by -2^-20 * idepth px — off the lower borders, just inside the upper ones
    s2 = _source([(4, 24), (24, 4), (W - 5, 26), (26, H - 5)], [1.0] * 4)
    hit(W - 5, 26), hit(26, H - 5)
    # source 3: t = (+2^-28, +2^-28, 0): off the upper borders, just inside the lower ones; 14 more on (40, 30); the second on (50, 40)
    uv3 = [(W - 5, 28), (28, H - 5), (4, 30), (30, 4)] + [(40, 30)] * 14 + [(50, 40)]
    rho3 = [1.0] * 4 + [(j + 1) / 8.0 for j in range(14)] + [1.5]
    hit(4, 30), hit(30, 4), hit(40, 30, 14), hit(50, 40)
    s3 = _source(uv3, rho3)
    # source 4: t_z = -2, used only for this: z = 1 - 2 idepth is 0, negative, and 1 / 2 (lands on (54, 38) with depth scale 1 / 2)
    s4 = _source([(30, 36), (33, 36), (46.25, 33.75)], [0.5, 1.0, 0.25])
    hit(54, 38)
    poses = [_pose((0, 0, 0)), _pose((2.0 ** -9, 2.0 ** -10, 0)), _pose((-2.0 ** -28, -2.0 ** -28, 0)), _pose((2.0 ** -28, 2.0 ** -28, 0)),
             _pose((0, 0, -2.0)), _pose((0, 0, 0))]
    return dict(kind="exact", W=W, H=H, levels=5, intr=_exact_intr(W, H), poses=poses, sources=[s0, s1, s2, s3, s4], variance="constant",
                expect=expect, isolated=(20, 45), stacked=((40, 30), 64), zero_sum_cells=((8, 8), (11, 8), (14, 8)))


def _grid_case(W, H, levels, counts, seed, occupancy=None, tail_rows=0):
    """exact, no motion: source i takes counts[i] distinct ROI pixels drawn without replacement (all of them in row-major order when
    `occupancy` is 1), so every occupied cell is hit once; tail_rows: the last source also takes every ROI pixel of the last rows"""
    rng = np.random.default_rng(seed)
    cells = _roi_cells(W, H)
    if occupancy is not None:
        total = int(round(occupancy * len(cells)))
        counts = [total // len(counts) + (1 if i < total % len(counts) else 0) for i in range(len(counts))]
    if tail_rows:
        tail = cells[cells[:, 1] >= H - BORDER - tail_rows]
        cells = cells[cells[:, 1] < H - BORDER - tail_rows]
    order = np.arange(len(cells)) if sum(counts) == len(cells) else rng.permutation(len(cells))[:sum(counts)]
    sources, o = [], 0
    for i, n in enumerate(counts):
        uv = cells[order[o:o + n]]
        o += n
        if tail_rows and i == len(counts) - 1:
            uv = np.concatenate([uv, tail])
        sources.append(_source(uv, _dyadic_idepth(len(uv), rng)))
    return dict(kind="exact", W=W, H=H, levels=levels, intr=_exact_intr(W, H), poses=[_pose((0, 0, 0))] * (len(counts) + 1), sources=sources,
                variance="constant", hits_once=True)


def _capacity():
    """360 x 280 x 1: a full window (16 keyframes, 15 sources) whose first 66 900 ROI pixels in row-major order go to the sources in turn:
    the splat batch is full, and the level holds more than 65 536 reference points"""
    W, H, n_sources, total = 360, 280, 15, 66900
    cells = _roi_cells(W, H)[:total]
    idx = np.arange(total)
    sources = [_source(cells[idx % n_sources == i], (1 + (idx[idx % n_sources == i] % 16)) / 16.0) for i in range(n_sources)]
    return dict(kind="exact", W=W, H=H, levels=1, intr=_exact_intr(W, H), poses=[_pose((0, 0, 0))] * (n_sources + 1), sources=sources,
                variance="constant", hits_once=True, min_points=65537)


def _general(W, H, levels, seed, variance, n_per_source=(300, 300, 300, 300)):
    """seeded random motion of the size synthetic.BASE_MOTION produces, integer uv, a tenth of the landmarks flagged or without status OK"""
    from dsopp_amd import synthetic as syn
    rng = np.random.default_rng(seed)
    poses = [syn.mat_to_params(syn.se3_exp(i * syn.BASE_MOTION + np.concatenate([rng.normal(0, 2e-2, 3), rng.normal(0, 5e-3, 3)])))
             for i in range(len(n_per_source) + 1)]
    sources = []
    for n in n_per_source:
        uv = np.stack([rng.integers(BORDER, W - BORDER, n), rng.integers(BORDER, H - BORDER, n)], axis=1)
        sources.append(_source(uv, rng.uniform(0.2, 1.5, n), (rng.random(n) < 0.1) * rng.integers(1, 4, n), (rng.random(n) < 0.1) * rng.integers(1, 4, n)))
    return dict(kind="general", W=W, H=H, levels=levels, intr=np.array([0.9 * W, 0.95 * W, 0.5 * W - 0.3, 0.5 * H + 0.2]), poses=poses, sources=sources,
                variance=variance, image_seed=seed + 100)


CASES = {
    "edges": _edges,                                                                               # 77 x 59 x 5
    "ragged": lambda: _grid_case(77, 59, 5, [0, 1, 255, 256, 257, 700], seed=1),                   # landmark counts around the 256-thread workgroup
    "full": lambda: _grid_case(48, 48, 5, [1000, 600], seed=2, occupancy=1.0),                     # every ROI cell occupied; coarsest level 3 x 3
    "sparse": lambda: _grid_case(131, 37, 3, [20, 15], seed=3, occupancy=0.01),                    # ~1 % occupied; second, partial dilation block
    "half": lambda: _grid_case(300, 41, 2, [1, 1, 1], seed=4, occupancy=0.5),                      # second 256-column chunk of compaction and flow
    "tall": lambda: _grid_case(24, 4120, 2, [1, 1], seed=5, occupancy=0.25, tail_rows=12),         # 258 flow strips; 17 rows per scan thread
    "capacity": _capacity,                                                                         # 360 x 280 x 1
    "general_const": lambda: _general(300, 41, 2, seed=11, variance="constant"),
    "general_readback_77": lambda: _general(77, 59, 5, seed=12, variance="readback"),
    "general_readback_131": lambda: _general(131, 37, 3, seed=13, variance="readback"),
}


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    c["name"] = name
    assert len(c["poses"]) == len(c["sources"]) + 1
    return c


@functools.lru_cache(maxsize=None)
def constant_variance_maps(name):
    """(dilated levels, Splat) of a case at the constant variance: computed once, shared by the tests, never written to"""
    maps, s = case_maps(case(name))
    for a in [m for lv in maps for m in lv] + [s.ids, s.wgt, s.k]:
        a.setflags(write=False)
    return maps, s
