"""Scenes for the landmark activator and the one way they reach the device, shared by tests/test_landmark_activation.py,
tests/test_activation_model.py (CPU: model against oracle) and tests/test_gpu_activation_edges.py (device against model).

A scene is a dict: name, frames (the oracle's layout plus `active_flags`, see activation_model), intr, ms (mask of the newest keyframe at the
sparsity level or None), desired, dist0, refine, sigma, exact.

EXACT scenes: identity poses, fx = fy = 256 with dyadic cx, cy, `desired` equal to the counted active landmarks.  K1 [R|t] K1^-1 is then the
identity in binary64 on every side and z = 1, so a landmark whose level-0 projection is 2p lands at exactly p on the sparsity level, the
regulated distance equals the input distance bit for bit, and statuses follow from the placement alone — ties included."""
import copy

import numpy as np

import activation_model as am
from dsopp_amd import synthetic as syn

W, H = 320, 240
IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.float64)


def _rel(T_w_t, T_w_r):
    return np.linalg.inv(T_w_t) @ T_w_r


def build_case(num_frames=5, per_frame=260, seed=83, observe=True, width=W, height=H, n_active=100, n_skip=7):
    """a window of `num_frames` keyframes (the last one is the new keyframe without landmarks); the first `n_active` landmarks of
    every older keyframe are active, the others immature with the estimator state two depth-estimation passes leave"""
    from oracle import pyoracle as po
    win = syn.make_window(num_frames=num_frames, num_points=num_frames * per_frame, width=width, height=height, seed=seed, pose_noise=False,
                          affine_jitter=True)
    intr = win.scene.intrinsics
    rng = np.random.default_rng(seed)
    frames = []
    for i, f in enumerate(win.frames):
        # the images are rendered as exp(a) * texture + b with exposure 1; a non-trivial exposure is folded out of `a` so that
        # (e_t / e_r) * exp(a_t - a_r) stays the true brightness ratio
        expo = 1.0 + 0.05 * i
        d = dict(pixelinfo=f.pixelinfo, mask=None, T_w=syn.mat_to_params(f.T_w_c_gt), exposure=expo,
                 affine=np.array([f.affine_gt[0] - np.log(expo), f.affine_gt[1]]), syn=f)
        if i + 1 < num_frames:
            na = n_active
            d["active_uv"], d["active_idepth"] = f.uv[:na].copy(), f.idepth_init[:na].copy()
            skip = np.zeros(na, dtype=np.uint8)
            skip[rng.choice(na, n_skip, replace=False)] = 1
            d["active_skip"] = skip
            d["active_patch"] = f.patch[:na].copy()
            uv = f.uv[na:]
            ui, vi = uv[:, 0].astype(int), uv[:, 1].astype(int)
            grad = np.stack([f.pixelinfo[vi, ui, 1], f.pixelinfo[vi, ui, 2]], axis=1)
            direction = np.stack([(uv[:, 0] - intr[2]) / intr[0], (uv[:, 1] - intr[3]) / intr[1], np.ones(len(uv))], axis=1)
            lms = po.new_immature_landmarks(uv, direction, f.patch[na:], grad)
            if observe:   # two observations from later keyframes give the intervals / uniqueness a realistic spread
                for j in (i + 1, num_frames - 1):
                    if j == i or j >= num_frames:
                        continue
                    g = win.frames[j]
                    po.estimate_depths(lms, g.pixelinfo, None, intr, syn.mat_to_params(_rel(g.T_w_c_gt, f.T_w_c_gt)), d["exposure"], d["affine"],
                                       1.0 + 0.05 * j, np.array([g.affine_gt[0] - np.log(1.0 + 0.05 * j), g.affine_gt[1]]))
            d["immature"] = lms
            d["idepth_gt"] = f.idepth_gt[na:].copy()
        frames.append(d)
    return win, frames, intr


def gpu_flags(f):
    """the flag bytes set_landmarks takes (bit 1 marginalised, bit 2 outlier): `active_flags`, or the skipped landmarks of `active_skip` as
    marginalised and outliers in turn"""
    if f.get("active_flags") is not None:
        return np.asarray(f["active_flags"], dtype=np.uint8)
    return (f["active_skip"] * (1 + (np.arange(len(f["active_skip"])) % 2))).astype(np.uint8)


def load_gpu(g, frames, intr):
    """the older keyframes into a HipWindow; -> their immature sets (None where a keyframe has none)"""
    from dsopp_amd import capi
    sets = []
    for i, f in enumerate(frames[:-1]):
        g.push_frame(i, 1000 * (i + 1), f["pixelinfo"], f.get("mask"), intr, f["T_w"], f["exposure"], f["affine"], i == 0, False)
        g.set_landmarks(i, f["active_uv"], f["active_idepth"], f["active_patch"], gpu_flags(f))
        if f.get("immature") is None:
            sets.append(None)
            continue
        s = capi.ImmatureSet(f["immature"])
        s.upload(f["immature"])
        sets.append(s)
    for i in range(len(frames) - 1):
        for j in range(len(frames) - 1):
            if i != j and len(frames[i]["active_idepth"]):
                g.set_connection(i, j, np.zeros(len(frames[i]["active_idepth"]), dtype=np.uint8))
    return sets


def newest_pyramid(frames, ms, dtype):
    from dsopp_amd import capi
    new = frames[-1]
    height, width = new["pixelinfo"].shape[:2]
    pyr = capi.Pyramid(width, height, 2, dtype)
    pyr.set_level(0, new["pixelinfo"])
    if new.get("mask") is not None:
        pyr.set_mask(0, new["mask"])
    if ms is not None:
        pyr.set_mask(1, ms)
    return pyr


def activate_gpu(g, frames, sets, pyr, desired, dist0, refine, sigma=20.0, ids=None):
    """one call on a loaded window (ids: the window's frame ids of frames[:-1], default 0, 1, ..); -> (statuses, idepths, result, downloaded
    set states)"""
    new = frames[-1]
    st, idp, res = g.activate_landmarks(list(range(len(frames) - 1)) if ids is None else ids, sets, pyr, new["T_w"], new["exposure"], new["affine"], desired, dist0, refine, sigma)
    return st, idp, res, [None if s is None else s.download() for s in sets]


def run_gpu(frames, intr, ms, desired, dist0, refine, dtype=None, sigma=20.0):
    from dsopp_amd import capi
    opts = capi.default_pba_options()
    if dtype is not None:
        opts.dtype = dtype
    g = capi.HipWindow(opts)
    sets = load_gpu(g, frames, intr)
    pyr = newest_pyramid(frames, ms, opts.dtype)
    out = activate_gpu(g, frames, sets, pyr, desired, dist0, refine, sigma)
    for s in sets:
        if s is not None:
            s.close()
    pyr.close()
    g.close()
    return out


def run_scene_gpu(sc, dtype=None):
    return run_gpu(sc["frames"], sc["intr"], sc["ms"], sc["desired"], sc["dist0"], sc["refine"], dtype, sc["sigma"])


def oracle_frames(frames):
    """the frames as the oracle's interface takes them: active_skip = isOutlier() || isMarginalized() and the inverse depth of the keyframe's
    landmark, both AFTER updateFrame's rules (activation_model.active_rules); an absent immature set as an empty one"""
    out = copy.deepcopy(frames)
    for f in out[:-1]:
        flags = am.active_flags(f)
        rules = [am.active_rules(r, int(g)) for r, g in zip(f["active_idepth"], flags)]
        f["active_idepth"] = np.array([r for r, _ in rules], dtype=np.float64)
        f["active_skip"] = np.array([not c for _, c in rules], dtype=np.uint8)
        if f.get("immature") is None:
            f["immature"] = immature_at(np.zeros((0, 2)))
    return out


_MODEL = {}


def model(sc, **kw):
    """the model's result of a scene, computed once per variant"""
    key = (sc["name"],) + tuple(sorted((k, getattr(v, "__name__", v)) for k, v in kw.items()))
    if key not in _MODEL:
        _MODEL[key] = am.activate(sc["frames"], sc["intr"], sc["sigma"], sc["desired"], sc["dist0"], sc["refine"], sc["ms"], **kw)
    return _MODEL[key]


# ---------------------------------------------------------------------------------------------------------------------------------------
# exact scenes
# ---------------------------------------------------------------------------------------------------------------------------------------
def immature_at(points, status=am.IMM_GOOD, traced=1, interval=1.0, uniqueness=10.0, idepth_min=1.0, idepth_max=1.0):
    """ready landmarks whose level-0 projections are twice `points` (n x 2, sparsity level); every keyword takes a scalar or n values"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    n = len(p)
    lms = syn.new_immature_landmarks(2.0 * p, np.concatenate([np.zeros((n, 2)), np.ones((n, 1))], axis=1), np.zeros((n, 8)), np.ones((n, 2)))
    full = lambda v, dt: np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dt), (n,))).copy()   # noqa: E731
    lms.update(status=full(status, np.uint8), traced=full(traced, np.uint8), search_pixel_interval=full(interval, np.float64),
               uniqueness=full(uniqueness, np.float64), idepth_min=full(idepth_min, np.float64), idepth_max=full(idepth_max, np.float64))
    return lms


def exact_scene(name, keyframes, dist0, width=128, height=96, ms=None, desired_offset=0, cx=None, cy=None):
    """keyframes: one (active, immature) per older keyframe — active: rows (x, y, idepth, flags) at the sparsity level, immature: the struct of
    arrays (immature_at) or None.  `desired` is the counted active landmarks plus desired_offset."""
    blank = np.zeros((height, width, 3))
    frames, counted = [], 0
    for active, immature in keyframes:
        a = np.asarray(active, dtype=np.float64).reshape(-1, 4)
        flags = a[:, 3].astype(np.uint8)
        counted += sum(am.active_rules(r, int(g))[1] for r, g in zip(a[:, 2], flags))
        frames.append(dict(pixelinfo=blank, mask=None, T_w=IDENTITY.copy(), exposure=1.0, affine=np.zeros(2), active_uv=2.0 * a[:, :2],
                           active_idepth=a[:, 2].copy(), active_flags=flags, active_patch=np.zeros((len(a), 8)), immature=immature))
    frames.append(dict(pixelinfo=blank, mask=None, T_w=IDENTITY.copy(), exposure=1.0, affine=np.zeros(2)))
    intr = np.array([256.0, 256.0, width / 2.0 if cx is None else cx, height / 2.0 if cy is None else cy])
    return dict(name=name, frames=frames, intr=intr, ms=ms, desired=counted + desired_offset, dist0=float(dist0), refine=False, sigma=20.0,
                exact=desired_offset == 0)


def _active(points, idepth=0.5, flags=0):
    return [(x, y, idepth, flags) for x, y in points]


def tie_scenes():
    """sites 12 apart (more than twice any distance used): the 3-4-5 pair, a coincident pair, a candidate on an active landmark, and the same
    under every kind of active landmark that must not block it"""
    site = lambda k: (8.0 + 12.0 * (k % 4), 8.0 + 12.0 * (k // 4))   # noqa: E731
    # active landmark kinds: plain (blocks), outlier-flagged, marginalised-flagged, negative inverse depth (none of the three is counted),
    # idepth >= 1010 (counted, not kept), |idepth| < 1e-8 of either sign (flushed to 0: counted, kept, blocks)
    kinds = [(0.5, 0), (0.5, am.FLAG_OUTLIER), (0.5, am.FLAG_MARGINALIZED), (-0.5, 0), (1010.0, 0), (-5e-9, 0), (5e-9, 0), (0.5, am.FLAG_OUTLIER | am.FLAG_MARGINALIZED)]
    active = [site(2 + k) + kind for k, kind in enumerate(kinds)]
    x0, y0 = site(0)
    x1, y1 = site(1)
    cand = [(x0, y0), (x0 + 3.0, y0 + 4.0), (x1, y1), (x1, y1)] + [site(2 + k) for k in range(len(kinds))]
    out = []
    for name, d in (("d5", 5.0), ("d5next", float(np.nextafter(5.0, 10.0))), ("d0", 0.0), ("d5prev", float(np.nextafter(5.0, 0.0)))):
        # the active landmarks in the first keyframe, the candidates split over two so that the pairs straddle the set boundary
        out.append(exact_scene("ties_" + name, [(active, immature_at(cand[:3])), ([], immature_at(cand[3:]))], d))
    return out


def _serpentine(d, n_rows, x0=4.0, x1=59.0, y0=6.0):
    """a path of points 0.75 d apart: rows 1.5 d apart, joined at alternating ends by one point half-way"""
    step, pts = 0.75 * d, []
    per_row = int((x1 - x0) / step) + 1
    for r in range(n_rows):
        xs = [x0 + step * k for k in range(per_row)]
        y = y0 + 2 * step * r
        pts += [(x, y) for x in (xs if r % 2 == 0 else xs[::-1])]
        if r + 1 < n_rows:
            pts.append((pts[-1][0], y + step))
    return pts


def chain_scenes():
    pts = _serpentine(1.0, 5)                      # 5 rows of 74 and 4 joints: 374 candidates, every one within the distance of the previous
    assert len(pts) >= 300 and max(p[1] for p in pts) <= 43.0
    rng = np.random.default_rng(7)
    orders = dict(forward=np.arange(len(pts)), reverse=np.arange(len(pts))[::-1], shuffled=rng.permutation(len(pts)))
    out = []
    for name, order in orders.items():
        p = np.array(pts)[order]
        cut = (125, 250)
        out.append(exact_scene("chain_" + name, [([], immature_at(p[:cut[0]])), ([], immature_at(p[cut[0]:cut[1]])), ([], immature_at(p[cut[1]:]))], 1.0))
    return out


def cluster_scenes():
    rng = np.random.default_rng(11)
    d = 8.0
    pts = []
    while len(pts) < 40:                           # 40 candidates inside a circle of radius d / 2 (coordinates on a 1/8 grid)
        x, y = rng.integers(-32, 33, 2) / 8.0
        if x * x + y * y < 16.0:
            pts.append((30.0 + x, 22.0 + y))
    out = [exact_scene("cluster_disc", [([], immature_at(pts[:17])), ([], immature_at(pts[17:]))], d)]
    for k in (12, 13):
        # A accepted; k candidates 0.9 d .. 0.95 d from it, within d of A and of each other: all blocked; Z at 1.8125 d: within d of every one of
        # the k and of nothing else, so it is ACCEPTED although its earlier neighbours fill (k = 12) or overflow (k = 13) the neighbour list
        row = [(10.0, 20.0)] + [(10.0 + 7.25 + j / 64.0, 20.0) for j in range(k)] + [(10.0 + 14.5, 20.0)]
        out.append(exact_scene("cluster_through_%d" % k, [([], immature_at(row[:5])), ([], immature_at(row[5:]))], d))
    return out


def workcap_scenes():
    """disjoint close pairs: exactly 8 and exactly 9 candidates wait on an earlier one after the neighbour pass, plus singles"""
    out = []
    for n in (8, 9):
        pts = []
        for k in range(n):
            x, y = 6.0 + 5.0 * k, 10.0 + 8.0 * (k % 3)
            pts += [(x, y), (x + 0.5, y + 0.25)]
        pts += [(8.0 + 5.0 * k, 40.0) for k in range(6)]
        out.append(exact_scene("workcap_%d" % n, [([], immature_at(pts[:7])), ([], immature_at(pts[7:]))], 1.0))
    return out


def _grid_points(d, sw, sh):
    """pairs closer than the distance that straddle a cell edge (cell = max(d, 4)) horizontally, vertically and diagonally, pairs in the
    first and last cell column and row of the ROI, and a pair exactly 4 apart"""
    cell = max(d, 4.0)
    s = min(d, 4.0) / 4.0 if d > 0 else 0.25
    ex, ey = cell * 2.0, cell * 2.0                # a cell edge in x and in y
    x_hi, y_hi = sw - 5.0, sh - 5.0
    pts = [(ex - s, 30.0), (ex + s, 30.0),                         # horizontal
           (34.0, ey - s), (34.0, ey + s),                         # vertical
           (cell * 3.0 - s, cell * 3.0 - s), (cell * 3.0 + s, cell * 3.0 + s),   # diagonal
           (cell * 3.0 + s, cell - s + 4.0), (cell * 3.0 - s, cell + s + 4.0),   # anti-diagonal
           (4.0, 17.0), (4.0 + s, 17.0), (x_hi, 25.0), (x_hi - s, 25.0),     # first / last column of the ROI
           (45.0, 4.0), (45.0, 4.0 + s), (41.0, y_hi), (41.0, y_hi - s),     # first / last row
           (4.0, 4.0), (4.0 + s, 4.0 + s), (x_hi, y_hi), (x_hi - s, y_hi - s),   # corners
           (50.0, 12.0), (54.0, 12.0)]                             # exactly 4 apart
    return pts


def grid_scenes():
    ulp4 = float(np.nextafter(4.0, 8.0))
    out = []
    for name, d in (("d0.5", 0.5), ("d4", 4.0), ("d4ulp", ulp4), ("d10", 10.0)):
        p = _grid_points(d, 64.0, 48.0)
        out.append(exact_scene("grid_" + name, [(_active([(20.0, 38.0)]), immature_at(p[:9])), ([], immature_at(p[9:]))], d))
    p = _grid_points(10.0, 64.0, 48.0)
    # (one counted active landmark against none desired: 9.9995 + 0.001 clamps to 10; 0.3 + (1 - 1001) * 0.001 clamps to 0)
    out.append(exact_scene("grid_clamp10", [(_active([(20.0, 38.0)]), immature_at(p[:9])), ([], immature_at(p[9:]))], 9.9995, desired_offset=-1))
    out.append(exact_scene("grid_clamp0", [(_active([(20.0, 38.0)]), immature_at(p[:9])), ([], immature_at(p[9:]))], 0.3, desired_offset=1000))
    # an odd half-size (130 x 98: the sparsity level is 65 x 49) and an odd level-0 width (129: the sparsity camera is 64.5 wide, its mask 64)
    p = _grid_points(4.0, 65.0, 49.0)
    out.append(exact_scene("grid_130x98", [(_active([(20.0, 38.0)]), immature_at(p[:9])), ([], immature_at(p[9:]))], 4.0, width=130, height=98))
    p = _grid_points(4.0, 64.5, 48.0) + [(float(np.nextafter(59.5, 100.0)), 33.0)]   # (the last: one ulp outside the fractional ROI edge)
    out.append(exact_scene("grid_129x96", [(_active([(20.0, 38.0)]), immature_at(p[:9])), ([], immature_at(p[9:]))], 4.0, width=129, height=96))
    return out


def mask_scenes():
    """CameraMask::valid rounds halves away from zero: (10.5, 7.5) reads mask pixel (11, 8)"""
    pts = [(10.5, 7.5), (30.0, 20.0)]
    only = np.full((48, 64), 255, dtype=np.uint8)
    only[8, 11] = 0
    others = np.full((48, 64), 255, dtype=np.uint8)
    others[7, 10] = others[8, 10] = others[7, 11] = 0
    return [exact_scene("mask_half_hit", [(_active(pts), immature_at(pts))], 0.0, ms=only),
            exact_scene("mask_half_miss", [(_active(pts), immature_at(pts))], 0.0, ms=others)]


def status_table_scene():
    """every status x traced x {ready, interval 8, uniqueness 3, midpoint 0, on the ROI edge u/2 = 4, on the edge u/2 = W/2 - 5, one ulp outside
    an edge}: one landmark per combination, 3 apart with the distance at 0.5"""
    pts, kw = [], dict(status=[], traced=[], interval=[], uniqueness=[], idepth_min=[], idepth_max=[])
    for s in range(7):
        for traced in (0, 1):
            y = 4.0 + 3.0 * (2 * s + traced)
            outside = float(np.nextafter(59.0, 100.0)) if (s + traced) % 2 else float(np.nextafter(4.0, 0.0))
            for c, x in enumerate((10.0, 16.0, 22.0, 28.0, 4.0, 59.0, outside)):
                pts.append((x, y))
                kw["status"].append(s)
                kw["traced"].append(traced)
                kw["interval"].append(8.0 if c == 1 else 1.0)
                kw["uniqueness"].append(3.0 if c == 2 else 10.0)
                kw["idepth_min"].append(-1.0 if c == 3 else 1.0)
                kw["idepth_max"].append(1.0)
    n = len(pts)   # (a landmark one ulp outside is no candidate: it cannot block the one ON the edge beside it)
    lm = immature_at(pts, **{k: np.array(v) for k, v in kw.items()})
    cut = lambda a, b: {k: v[a:b].copy() for k, v in lm.items()}   # noqa: E731
    return [exact_scene("status_table", [([], cut(0, n // 2)), ([], cut(n // 2, n))], 0.5)]


def _random_points(rng, n):
    return np.stack([rng.integers(16, 237, n) / 4.0, rng.integers(16, 173, n) / 4.0], axis=1)   # a 1/4 grid inside the ROI [4, 59] x [4, 43]


def count_scenes():
    """n_active and n_immature at 0, 1, the wave and the 256-thread block edges, a keyframe without a set in the middle, a single keyframe"""
    rng = np.random.default_rng(5)

    def kf(n_active, n_immature):
        a = _active(_random_points(rng, n_active)) if n_active else []
        return a, (None if n_immature is None else immature_at(_random_points(rng, n_immature)))

    table = dict(a=[(0, 1), (1, None), (63, 255)], b=[(64, 256), (65, 0), (256, 257)], large=[(257, 257), (0, None), (257, 1)],
                 single=[(257, 257)], single_1=[(1, 1)], single_0=[(0, 0)], empty=[(0, 0), (0, None), (0, 0)], small=[(3, 5), (2, 4)])
    out = []
    for name, counts in table.items():
        if name == "empty":   # no landmark of either kind anywhere: the distance is regulated from 0 active points, 1.5 + (0 - 700) * 0.001
            out.append(exact_scene("counts_empty", [kf(*c) for c in counts], 1.5, desired_offset=700))
        else:                 # (points on a 1/4 grid with the distance at 0.5: pairs exactly the distance apart occur, exactly)
            out.append(exact_scene("counts_" + name, [kf(*c) for c in counts], 0.5))
    return out


def selection_scenes():
    return tie_scenes() + chain_scenes() + cluster_scenes() + workcap_scenes() + grid_scenes() + mask_scenes() + status_table_scene() + count_scenes()


# ---------------------------------------------------------------------------------------------------------------------------------------
# refinement scenes: real baselines, 128 x 96
# ---------------------------------------------------------------------------------------------------------------------------------------
RW, RH = 128, 96
_CASES = {}


def _refine_case(num_frames, seed):
    if (num_frames, seed) not in _CASES:
        _CASES[(num_frames, seed)] = build_case(num_frames=num_frames, per_frame=55, seed=seed, width=RW, height=RH, n_active=10, n_skip=1)
    return _CASES[(num_frames, seed)]


def _refine_scene(name, num_frames, seed, dist0=2.0, sigma=20.0, edit=None):
    _, frames, intr = _refine_case(num_frames, seed)
    frames = [{k: v for k, v in f.items() if k != "syn"} for f in copy.deepcopy(frames)]
    if edit is not None:
        edit(frames)
    counted = sum(int((f["active_skip"] == 0).sum()) for f in frames[:-1])
    return dict(name=name, frames=frames, intr=np.asarray(intr, dtype=np.float64), ms=None, desired=counted, dist0=dist0, refine=True, sigma=sigma,
                exact=False)


def _zero_baseline(frames):
    """every keyframe at the identity pose over ONE image, the patches read from it: residuals vanish (targets are valid inliers) and, the
    translations being exactly zero, so does every derivative — the Hessian is exactly 0"""
    first = frames[0]
    for f in frames:
        f["T_w"] = IDENTITY.copy()
        f["pixelinfo"], f["exposure"], f["affine"] = first["pixelinfo"], first["exposure"], first["affine"].copy()
        if f.get("immature") is not None:
            u, v = f["immature"]["projection"][:, 0].astype(int), f["immature"]["projection"][:, 1].astype(int)
            f["immature"]["patch"] = np.stack([first["pixelinfo"][v + oy, u + ox, 0] for ox, oy in am.PATTERN], axis=1)


def _masks_zero(frames):
    for f in frames:
        f["mask"] = np.zeros(f["pixelinfo"].shape[:2], dtype=np.uint8)


def _wrong_exposure(frames):
    frames[2]["exposure"] = 4.0 * frames[2]["exposure"]


SEED = 83


def refinement_scenes():
    out = [_refine_scene("refine_F%d" % n, n, SEED) for n in (9, 10, 11, 16)]
    out.append(_refine_scene("refine_F2", 2, SEED))
    out.append(_refine_scene("refine_zero_baseline", 5, SEED, edit=_zero_baseline))
    out.append(_refine_scene("refine_masks_zero", 5, SEED, edit=_masks_zero))
    out.append(_refine_scene("refine_wrong_exposure", 5, SEED, edit=_wrong_exposure))
    out.append(_refine_scene("refine_huber", 5, SEED, sigma=1.0))
    return out


_SCENES = {}


def scenes(kind):
    """kind: "selection" or "refinement"; built once"""
    if kind not in _SCENES:
        _SCENES[kind] = {s["name"]: s for s in (selection_scenes() if kind == "selection" else refinement_scenes())}
    return _SCENES[kind]


SELECTION_NAMES = ["ties_d5", "ties_d5next", "ties_d0", "ties_d5prev", "chain_forward", "chain_reverse", "chain_shuffled", "cluster_disc",
                   "cluster_through_12", "cluster_through_13", "workcap_8", "workcap_9", "grid_d0.5", "grid_d4", "grid_d4ulp", "grid_d10", "grid_clamp10",
                   "grid_clamp0", "grid_130x98", "grid_129x96", "mask_half_hit", "mask_half_miss", "status_table", "counts_a", "counts_b", "counts_large",
                   "counts_single", "counts_single_1", "counts_single_0", "counts_empty", "counts_small"]
REFINEMENT_NAMES = ["refine_F9", "refine_F10", "refine_F11", "refine_F16", "refine_F2", "refine_zero_baseline", "refine_masks_zero",
                    "refine_wrong_exposure", "refine_huber"]
