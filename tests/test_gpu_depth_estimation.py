"""Row f-1 at production sizes and edges: the HIP depth estimator of immature landmarks against the CPU oracle (oracle/
depth_estimation.hpp) on rendered scenes of 640x480, 1280x1024 and an odd 643x481, with f64 and f32 texels, with and without
a camera mask, over observation sequences chosen for the kernel's less travelled paths: traced searches of several 64-point
passes (the carried minimum, the (energy, index) reduction across passes, LDS energies past index 63, the second-best scan),
forward / backward motion (epipole inside the image), pure x / pure y translation (the horizontal and vertical line branches),
pure rotation (no line), the depth-scale rejection and preset input states.  The batched call is checked with 8, 9 and 16
sets (9 is the first call of the pinned-table path, 16 its capacity).

The unmarked tests pin the generator: each scenario must reach what it exists for, so the GPU tests cannot quietly check
nothing after a change of the scenes.  The GPU tests hold the device to the oracle, fed with the texels the device stores."""
import copy
import functools

import numpy as np
import pytest

from dsopp_amd import synthetic as syn

SIZES = {"640x480": (640, 480), "1280x1024": (1280, 1024), "643x481": (643, 481)}
N_LANDMARKS = {"640x480": 2500, "1280x1024": 4000, "643x481": 1500}
MASKS = ("none", "pixel", "band")
STATUS = syn.IMMATURE_STATUS
RADIANCE = (0.55, 30.0)   # scene radiance = 0.55 * Scene.texture + 30 (the texture spans about -35 .. 290)


def _pose(t, w=(0.0, 0.0, 0.0)):
    return syn.se3_exp(np.r_[np.asarray(t, dtype=np.float64), np.asarray(w, dtype=np.float64)])


# observation sequences of the reference frame (camera at the identity): (T_world_target, exposure, affine (a, b)) per step
SCENARIOS = {
    # Every pose outside the axis sequence carries a small rotation.  With R = I and the integer landmark positions production
    # uses, the samples land on the pixel grid and on the ROI border exactly.  For example, at 640x480 with t = (0.008, 0.0024, 0)
    # and R = I, a pattern pixel of the landmark at (10, 190) reprojected to x = 3.9999999999999973 against the border at 4, and the
    # device and the oracle disagreed on whether that epipolar point had an energy at all.
    # short then long baseline: the second step traces intervals over segments of several 64-point passes; the third rotates more
    "baseline": [(_pose((0.008, 0.0024, 0.0), (0.001, -0.002, 0.0005)), 1.0, (0.0, 0.0)),
                 (_pose((0.8, -0.2, 0.1), (0.003, 0.01, -0.002)), 1.2, (0.04, 3.0)),
                 (_pose((0.6, 0.2, -0.05), (0.01, 0.0, 0.0)), 0.9, (-0.03, -4.0))],
    # epipole inside the image (limits_diff / borders_diff clipping); near landmarks fail the depth-scale test on the second step
    "forward": [(_pose((0.0, 0.0, 0.4), (0.002, 0.001, 0.0)), 1.0, (0.02, 1.5)),
                (_pose((0.02, 0.0, 1.2), (-0.002, 0.003, 0.001)), 1.1, (0.0, -2.0))],
    "backward": [(_pose((0.0, 0.0, -0.4), (0.001, 0.0, 0.002)), 1.0, (0.0, 0.0)),
                 (_pose((0.01, 0.01, -0.9), (0.0, -0.002, 0.001)), 0.95, (0.03, 2.0))],
    # R = I: pure y (b == 0, vertical line), then pure x (a == 0, slope 0) on the intervals traced by the first.  This sequence
    # observes landmarks at sub-pixel positions (World.axis_uv): with integer ones every sample of an axis-aligned line lies on the
    # pixel grid, energies are sums of integer squares, and equal energies at different points are decided by the last bit.  The x baseline is
    # not a whole multiple of the y one: with 0.15 = 3 x 0.05, fx = fy and errors capped at 10 px (intervals of whole pixels) the
    # traced segments were whole pixels long, e.g. 42.0 in the oracle and 41.99999999999999 on the other side of the rounding
    # (landmark 452 at 1280x1024), so getSize's floor gave 42 or 41 steps: a threshold straddle, not a kernel fault
    "axis": [(_pose((0.0, 0.05, 0.0)), 1.0, (0.0, 0.0)),
             (_pose((0.137, 0.0, 0.0)), 1.0, (-0.02, 1.0))],
    # |t| < 1e-3: no epipolar line at all
    "rotation": [(_pose((4e-4, 0.0, 0.0), (0.01, -0.02, 0.005)), 1.0, (0.0, 0.0))],
    # preset input states (statuses 0-6, mixed traced flags, intervals with idepth_min < 0 and empty ones), then two observations
    "state": [(_pose((0.3, -0.08, 0.05), (0.003, 0.01, -0.002)), 1.2, (0.04, 3.0)),
              (_pose((0.6, 0.2, -0.05), (0.01, 0.0, 0.0)), 0.9, (-0.03, -4.0))],
}
# the odd size only runs the sequence that reaches the long traced searches
SIZE_SCENARIOS = {"640x480": tuple(SCENARIOS), "1280x1024": tuple(SCENARIOS), "643x481": ("baseline",)}
LONG_STEP = ("baseline", 1)   # the long-baseline observation (coverage of multi-pass searches, ground-truth bracketing)


def _mask(kind, H, W, seed):
    """the mask shapes of test_gpu_masks.py"""
    if kind == "none":
        return None
    rng = np.random.default_rng(seed)
    if kind == "pixel":
        return (rng.random((H, W)) >= 0.15).astype(np.uint8) * 255
    m = np.full((H, W), 255, dtype=np.uint8)
    m[int(0.55 * H):int(0.55 * H) + 9, :] = 0                 # horizontal band
    m[:, int(0.3 * W):int(0.3 * W) + 5] = 0                   # vertical band
    for _ in range(12):                                       # blocks with odd sizes and offsets
        y, x = rng.integers(0, H - 20), rng.integers(0, W - 20)
        m[y:y + rng.integers(3, 20), x:x + rng.integers(3, 20)] = 0
    return m


def _inverse(T):
    """T^-1 of a rigid 4x4 (R^T, -R^T t): exact for R = I, so the pure-translation cases keep their zero components"""
    Ti = np.eye(4)
    Ti[:3, :3] = T[:3, :3].T
    Ti[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return Ti


def _u8(img):
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def _pick(pinfo, n, seed, subpixel=False):
    """n distinct pixels with |grad I| > 4, 8 px inside the image (as the feature extractor gives them: integer positions);
    subpixel: moved by offsets in [0.15, 0.85] (the axis sequence)"""
    H, W = pinfo.shape[:2]
    grad = np.hypot(pinfo[..., 1], pinfo[..., 2])
    vv, uu = np.nonzero(grad[8:H - 8, 8:W - 8] > 4.0)
    rng = np.random.default_rng(seed)
    pick = rng.choice(len(uu), min(n, len(uu)), replace=False)
    uv = np.stack([uu[pick] + 8.0, vv[pick] + 8.0], axis=1)
    return uv + rng.uniform(0.15, 0.85, uv.shape) if subpixel else uv


def _bilinear(img, u, v):
    x0, y0 = u.astype(int), v.astype(int)
    a, b = u - x0, v - y0
    return (1 - a) * (1 - b) * img[y0, x0] + a * (1 - b) * img[y0, x0 + 1] + (1 - a) * b * img[y0 + 1, x0] + a * b * img[y0 + 1, x0 + 1]


def _landmarks(pinfo, uv, intr):
    """new_immature_landmarks: patch and gradient sampled at the landmark (as test_depth_estimation._landmarks; bilinear for the
    sub-pixel positions)"""
    patch = np.stack([_bilinear(pinfo[..., 0], uv[:, 0] + ox, uv[:, 1] + oy) for ox, oy in syn.PATTERN], axis=1).reshape(len(uv), 8)
    grad = np.stack([_bilinear(pinfo[..., 1], uv[:, 0], uv[:, 1]), _bilinear(pinfo[..., 2], uv[:, 0], uv[:, 1])], axis=1).reshape(len(uv), 2)
    fx, fy, cx, cy = intr
    direction = np.stack([(uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy, np.ones(len(uv))], axis=1)
    return syn.new_immature_landmarks(uv, direction, patch, grad)


def _render(scene, T, exposure, a, b):
    """8-bit frame of radiance RADIANCE[0] * texture + RADIANCE[1] seen with (exposure, affine (a, b)).  The contrast keeps every
    frame clear of 0 and 255: on a saturated plateau neighbouring epipolar points have equal energies, decided by the last bit.
    (With the texture as rendered, at 640x480 the oracle's second-best / best energy of landmark 663 in the first step of the
    "state" sequence was 1.0000000000000004: four points with the energy 3064.88, and the device chose another of them.)"""
    s = exposure * np.exp(a)
    img, depth = scene.render_torch(T, float(np.log(s * RADIANCE[0])), s * RADIANCE[1] + b, "cpu")
    assert 0 < img.min() and img.max() < 255, (img.min(), img.max())
    return _u8(img), depth


class World:
    """one rendered scene per size: the reference frame (identity), every scenario's target frames, landmarks on the reference"""

    def __init__(self, size):
        W, H = SIZES[size]
        self.size, self.W, self.H = size, W, H
        self.scene = syn.Scene.make(W, H, 7)
        self.intr = self.scene.intrinsics
        self.ref_u8, depth = _render(self.scene, np.eye(4), 1.0, 0.0, 0.0)
        self.targets = {}
        for name in SIZE_SCENARIOS[size]:
            self.targets[name] = [_render(self.scene, T, e, a, b)[0] for T, e, (a, b) in SCENARIOS[name]]
        self.ref_pinfo = syn.pixelinfo_from_plane(self.ref_u8.astype(np.float64))
        self.uv = _pick(self.ref_pinfo, N_LANDMARKS[size], 11)
        self.axis_uv = _pick(self.ref_pinfo, N_LANDMARKS[size], 11, subpixel=True)
        self.idepth_gt = 1.0 / _bilinear(depth, self.uv[:, 0], self.uv[:, 1])

    def landmarks(self, scenario, idx=None):
        """new_immature_landmarks on the reference frame; the "state" scenario gets its preset input state"""
        uv = self.axis_uv if scenario == "axis" else self.uv
        uv = uv if idx is None else uv[idx]
        lms = _landmarks(self.ref_pinfo, uv, self.intr)
        if scenario == "state":
            rng = np.random.default_rng(5)
            n = len(uv)
            gt = self.idepth_gt if idx is None else self.idepth_gt[idx]
            lms["status"] = rng.integers(0, 7, n).astype(np.uint8)
            lms["traced"] = (rng.random(n) < 0.5).astype(np.uint8)
            lo = gt * rng.uniform(0.5, 1.0, n) - rng.uniform(0.1, 0.3, n) * (rng.random(n) < 0.2)   # most of these below zero
            hi = gt * rng.uniform(1.0, 1.6, n)
            swap = rng.random(n) < 0.05                                                          # idepth_max < idepth_min
            lms["idepth_min"], lms["idepth_max"] = np.where(swap, hi, lo), np.where(swap, lo, hi)
            lms["uniqueness"] = rng.uniform(0.5, 5.0, n)
            lms["search_pixel_interval"] = rng.uniform(0.0, 20.0, n)
        return lms

    def T_target_reference(self, scenario, step):
        return _inverse(SCENARIOS[scenario][step][0])

    def photometry(self, scenario, step):
        """(target exposure, target affine) of a step; the reference is (1, (0, 0))"""
        _, e, ab = SCENARIOS[scenario][step]
        return e, ab


@functools.lru_cache(maxsize=None)
def _world(size):
    return World(size)


@pytest.fixture(scope="module")
def worlds():
    return _world


# ---------------------------------------------------------------------------------------------------------------- oracle side

def _oracle_steps(world, scenario, texels, mask):
    """the oracle over a scenario: [(state before, state after)] per step; texels[step] = H x W x 3 target pixel info"""
    from oracle import pyoracle as po
    lms = world.landmarks(scenario)
    out = []
    for step in range(len(SCENARIOS[scenario])):
        pre = copy.deepcopy(lms)
        e, ab = world.photometry(scenario, step)
        po.estimate_depths(lms, texels[step], mask, world.intr, syn.mat_to_params(world.T_target_reference(scenario, step)), 1.0, (0.0, 0.0), e, ab)
        out.append((pre, copy.deepcopy(lms)))
    return out


@functools.lru_cache(maxsize=None)
def _host_run(size, scenario, kind):
    """oracle run on host-computed pixel info (the coverage pins: no device needed)"""
    w = _world(size)
    texels = [syn.pixelinfo_from_plane(u8.astype(np.float64)) for u8 in w.targets[scenario]]
    return _oracle_steps(w, scenario, texels, _mask(kind, w.H, w.W, 3))


def _searched_lengths(world, scenario, step, pre):
    """points of the epipolar segment each traced landmark searches in this step (findBest walks all of them when traced)"""
    from oracle import pyoracle as po
    T = syn.mat_to_params(world.T_target_reference(scenario, step))
    sel = np.flatnonzero((pre["traced"] == 1) & ~np.isin(pre["status"], (1, 2, 6)))
    n = np.zeros(len(sel), dtype=int)
    for j, i in enumerate(sel):
        proj, _ = po.build_epipolar_segment(world.W, world.H, world.intr, T, pre["projection"][i], pre["idepth_min"][i], pre["idepth_max"][i])
        n[j] = len(proj)
    return n


# ---------------------------------------------------------------------------------------------------------- coverage pins (CPU)

@pytest.mark.parametrize("size", ["640x480", "1280x1024", "643x481"])
def test_long_traced_searches_are_reached(worlds, size):
    """the long-baseline step searches traced segments of more than one and more than two 64-point passes"""
    w = worlds(size)
    pre, _ = _host_run(size, "baseline", "none")[LONG_STEP[1]]
    n = _searched_lengths(w, "baseline", LONG_STEP[1], pre)
    assert (n > 64).sum() >= 50 and (n > 128).sum() >= 10, (size, (n > 64).sum(), (n > 128).sum(), n.max())


@pytest.mark.parametrize("size", ["640x480", "1280x1024"])
def test_every_outcome_is_produced(worlds, size):
    """statuses 0-4 all come out of the scenarios; pure rotation leaves nothing but out-of-boundary"""
    seen = set()
    for name in SIZE_SCENARIOS[size]:
        for _, post in _host_run(size, name, "none"):
            seen |= set(post["status"].tolist())
    assert {0, 1, 2, 3, 4} <= seen, seen
    (_, rot), = _host_run(size, "rotation", "none")
    assert np.all(rot["status"] == STATUS["out_of_boundary"])
    pre, post = _host_run(size, "state", "none")[0]
    assert set(pre["status"].tolist()) == set(range(7)) and (pre["idepth_min"] < 0).sum() > 50
    keep = np.isin(pre["status"], (1, 2, 6))                    # never touched by the estimator
    assert np.array_equal(post["status"][keep], pre["status"][keep]) and np.array_equal(post["idepth_min"][keep], pre["idepth_min"][keep])
    assert (post["status"][~keep] == 0).sum() > 100


@pytest.mark.parametrize("size", ["640x480", "1280x1024"])
def test_axis_motion_gives_exact_vertical_and_horizontal_lines(worlds, size):
    """pure y with R = I: every landmark's line has start.x == end.x exactly (the b == 0 branch); pure x: start.y == end.y"""
    w = worlds(size)
    fx, fy, cx, cy = w.intr
    for step, axis in ((0, 0), (1, 1)):
        T = w.T_target_reference("axis", step)
        assert np.array_equal(T[:3, :3], np.eye(3)) and T[2, 3] == 0 and T[axis, 3] == 0
        # NumPy reprojection K [R|t] K^-1 at the two ends of the search range (inverse depth 1000 and 0)
        ends = []
        for rho in (1000.0, 0.0):
            d = np.stack([(w.axis_uv[:, 0] - cx) / fx, (w.axis_uv[:, 1] - cy) / fy, np.ones(len(w.axis_uv))], axis=1)
            X = d @ T[:3, :3].T + rho * T[:3, 3]
            ends.append(np.stack([fx * X[:, 0] / X[:, 2] + cx, fy * X[:, 1] / X[:, 2] + cy], axis=1))
        assert np.array_equal(ends[0][:, axis], ends[1][:, axis])
        assert np.all(ends[0][:, 1 - axis] != ends[1][:, 1 - axis])
    _, post = _host_run(size, "axis", "none")[0]
    assert (post["status"] == 0).sum() > 0.5 * len(w.axis_uv)


@pytest.mark.parametrize("size", ["640x480", "1280x1024"])
def test_forward_and_backward_epipoles_inside_the_image(worlds, size):
    """the epipole (the reference centre seen from the target) lies inside the image for both steps of forward and backward
    motion, and the forward sequence reaches the depth-scale rejection"""
    from oracle import pyoracle as po
    w = worlds(size)
    fx, fy, cx, cy = w.intr
    for name in ("forward", "backward"):
        for step in range(2):
            t = w.T_target_reference(name, step)[:3, 3]
            ex, ey = fx * t[0] / t[2] + cx, fy * t[1] / t[2] + cy
            assert 0 <= ex < w.W and 0 <= ey < w.H, (name, step, ex, ey)
    pre, post = _host_run(size, "forward", "none")[1]
    T = w.T_target_reference("forward", 1)
    rejected = 0
    for i in np.flatnonzero((pre["traced"] == 1) & (pre["idepth_min"] >= 0) & (post["status"] == 1)):
        proj, idp = po.build_epipolar_segment(w.W, w.H, w.intr, syn.mat_to_params(T), pre["projection"][i], pre["idepth_min"][i], pre["idepth_max"][i])
        if len(proj) > 2:
            scale = T[2, :3] @ pre["direction"][i] + T[2, 3] * idp[0]
            rejected += not (0.75 <= scale <= 1.5)
    assert rejected >= 20, rejected


@pytest.mark.parametrize("size", ["640x480", "1280x1024"])
def test_masks_change_outcomes(worlds, size):
    for kind in ("pixel", "band"):
        changed = 0
        for name in ("baseline", "forward"):
            for (_, a), (_, b) in zip(_host_run(size, name, "none"), _host_run(size, name, kind)):
                changed += int((a["status"] != b["status"]).sum() + ((a["status"] == 0) & (b["status"] == 0) & (a["idepth_min"] != b["idepth_min"])).sum())
        assert changed >= 50, (kind, changed)


# ------------------------------------------------------------------------------------------------------------- GPU parity

def _assert_parity(want, got, what, diag=None):
    """the bars of test_depth_estimation.test_gpu_depth_estimation_matches_oracle; diag = (world, state before, T, texels, mask,
    photometry) prints the first landmarks that differ in any field"""
    if diag is not None:
        differ = np.zeros(len(want["status"]), dtype=bool)
        for k in ("status", "traced", "idepth_min", "idepth_max", "search_pixel_interval", "uniqueness"):
            differ |= ~np.isclose(want[k], got[k], rtol=1e-7, atol=1e-8)
        for i in np.flatnonzero(differ)[:3]:
            print(_explain(i, want, got, what, *diag))
    bad = np.flatnonzero(want["status"] != got["status"])
    assert len(bad) == 0, (what, bad[:20], want["status"][bad[:20]], got["status"][bad[:20]])
    assert np.array_equal(want["traced"], got["traced"]), what
    for k in ("idepth_min", "idepth_max", "search_pixel_interval"):
        d = np.abs(want[k] - got[k])
        assert d.max(initial=0) <= 1e-8 * max(1.0, np.abs(want[k]).max(initial=0)), (what, k, int(np.argmax(d)), d.max())
    fin = want["uniqueness"] < 1e300
    assert np.array_equal(fin, got["uniqueness"] < 1e300), (what, np.flatnonzero(fin != (got["uniqueness"] < 1e300))[:20])
    if fin.any():
        rel = np.abs(want["uniqueness"][fin] - got["uniqueness"][fin]) / np.abs(want["uniqueness"][fin])
        assert rel.max() <= 1e-7, (what, np.flatnonzero(fin)[int(np.argmax(rel))], rel.max())


def _explain(i, want, got, what, world, pre, T, texels, mask, photometry):
    """a landmark whose outcome differs: its input state, both outcomes, and the NumPy energies (findBest's sum of squared
    residuals, invalid = inf) and inverse depths along the oracle's segment"""
    from oracle import pyoracle as po
    fx, fy, cx, cy = world.intr
    H, W = texels.shape[:2]
    e_t, (a_t, b_t) = photometry
    uv = pre["projection"][i]
    proj, idp = po.build_epipolar_segment(W, H, world.intr, syn.mat_to_params(T), uv, pre["idepth_min"][i], pre["idepth_max"][i])
    energies = np.full(len(proj), np.inf)
    for j, rho in enumerate(idp):
        d = np.stack([(uv[0] + syn.PATTERN[:, 0] - cx) / fx, (uv[1] + syn.PATTERN[:, 1] - cy) / fy, np.ones(8)], axis=1)
        X = d @ T[:3, :3].T + rho * T[:3, 3]
        u, v = fx * X[:, 0] / X[:, 2] + cx, fy * X[:, 1] / X[:, 2] + cy
        mx, my = int(np.round(proj[j][0])), int(np.round(proj[j][1]))
        if (-1e-4 < rho < 1010 and np.all(X[:, 2] > 0) and np.all((u >= 4) & (v >= 4) & (u <= W - 5) & (v <= H - 5))
                and 0 <= mx < W and 0 <= my < H and (mask is None or mask[my, mx] != 0)):
            r = (_bilinear(texels[..., 0], u, v) - b_t) - e_t * np.exp(a_t) * pre["patch"][i]
            energies[j] = np.sum(r * r)
    fields = ("status", "traced", "idepth_min", "idepth_max", "uniqueness", "search_pixel_interval")
    return (f"[{what}] landmark {i} at {uv}, input status {pre['status'][i]} traced {pre['traced'][i]} interval "
            f"[{pre['idepth_min'][i]!r}, {pre['idepth_max'][i]!r}]\n  oracle {[want[k][i] for k in fields]}\n  device {[got[k][i] for k in fields]}\n"
            f"  segment of {len(proj)} points {proj[:1]} .. {proj[-1:]}, energies:\n  {np.array2string(energies, precision=1, threshold=4000)}\n"
            f"  inverse depths {np.array2string(idp, precision=5, threshold=4000)}")


_DEVICE_ORACLE = {}


def _pyramid(world, u8, dtype, mask):
    """the target pyramid the way production builds it: build from the 8-bit image, then the camera mask"""
    from dsopp_amd import capi
    pyr = capi.Pyramid(world.W, world.H, 1, dtype)
    pyr.build(u8)
    if mask is not None:
        pyr.set_mask(0, mask)
    return pyr


def _gpu_cases():
    out = []
    for size in ("640x480", "1280x1024", "643x481"):
        for name in SIZE_SCENARIOS[size]:
            for dtype in ("f64", "f32"):
                for kind in MASKS:
                    out.append(pytest.param(size, name, dtype, kind, id=f"{size}-{name}-{dtype}-{kind}"))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("size,scenario,dtype,kind", _gpu_cases())
def test_gpu_estimate_matches_oracle(worlds, size, scenario, dtype, kind):
    """every step of the scenario: the one-shot device call from the oracle's state before the step against the oracle (fed
    with the texels the device stores and the same mask); the device-resident set driven over the whole sequence ends bitwise
    equal to the one-shot calls chained on their own results.  (f32 texels: the estimator still computes in f64, so the bars
    are the f64 bars.)"""
    from dsopp_amd import capi
    w = worlds(size)
    mask = _mask(kind, w.H, w.W, 3)
    pyrs = [_pyramid(w, u8, capi.F64 if dtype == "f64" else capi.F32, mask) for u8 in w.targets[scenario]]
    texels = [p.get_level(0) for p in pyrs]
    key = (size, scenario, kind)
    cached = _DEVICE_ORACLE.get(key)
    if cached is None or not all(np.array_equal(a, b) for a, b in zip(cached[0], texels)):
        cached = (texels, _oracle_steps(w, scenario, texels, mask))   # (u8 images: the f32 texels equal the f64 ones, one run serves both)
        _DEVICE_ORACLE[key] = cached
    steps = cached[1]
    chained = w.landmarks(scenario)
    dset = capi.ImmatureSet(w.landmarks(scenario))
    if scenario == "state":
        dset.upload(chained)
    try:
        for step, ((pre, want), pyr) in enumerate(zip(steps, pyrs)):
            T = w.T_target_reference(scenario, step)
            Tp = syn.mat_to_params(T)
            e, ab = w.photometry(scenario, step)
            got = copy.deepcopy(pre)
            capi.estimate_depths(got, pyr, 0, w.intr, Tp, 1.0, (0.0, 0.0), e, ab)
            _assert_parity(want, got, f"{size} {scenario} step {step} {dtype} mask {kind}", (w, pre, T, texels[step], mask, (e, ab)))
            if (scenario, step) == LONG_STEP:   # the physics, independently of the oracle: intervals bracket the rendered truth
                good = got["status"] == 0
                inside = (got["idepth_min"][good] <= w.idepth_gt[good] * 1.02) & (w.idepth_gt[good] * 0.98 <= got["idepth_max"][good])
                assert good.sum() > 0.5 * len(good) and inside.mean() >= 0.85, (good.sum(), inside.mean())
            capi.estimate_depths(chained, pyr, 0, w.intr, Tp, 1.0, (0.0, 0.0), e, ab)
            dset.estimate(pyr, 0, w.intr, Tp, 1.0, (0.0, 0.0), e, ab)
            st = dset.download()
            for k in st:
                assert np.array_equal(st[k], chained[k]), (step, k)
    finally:
        dset.close()
        for p in pyrs:
            p.close()


# ------------------------------------------------------------------------------------------------------------- GPU batched

BATCH_SIZE = "640x480"


def _batch_sets(w, n_sets, seed):
    """n_sets keyframe sets against one target, each on its own keyframe: the reference frame or a frame of the scenarios, with
    that frame's pose and photometry and landmarks picked on its image; sizes differ, one set is empty and one holds 1 landmark"""
    rng = np.random.default_rng(seed)
    frames = [(np.eye(4), 1.0, (0.0, 0.0), w.ref_u8)]
    for name in ("baseline", "forward", "backward", "axis"):
        frames += [(T, e, ab, u8) for (T, e, ab), u8 in zip(SCENARIOS[name], w.targets[name])]
    sizes = [int(x) for x in rng.integers(50, 800, n_sets)]
    sizes[1], sizes[-1] = 0, 1
    out = []
    for k in range(n_sets):
        T_w_r, e, ab, u8 = frames[k % len(frames)]
        pinfo = syn.pixelinfo_from_plane(u8.astype(np.float64))
        uv = _pick(pinfo, sizes[k], 100 + k)
        out.append(dict(lms=_landmarks(pinfo, uv, w.intr), T_w_r=T_w_r, e=e, ab=ab))
    return out


def _batch_oracle(w, sets, u8_target, T_w_t, e_t, ab_t, dtype):
    from oracle import pyoracle as po
    from dsopp_amd import capi
    pyr = _pyramid(w, u8_target, dtype, None)
    texels = pyr.get_level(0)
    Ts = np.stack([syn.mat_to_params(_inverse(T_w_t) @ s["T_w_r"]) for s in sets])
    want = []
    for s, T in zip(sets, Ts):
        lms = copy.deepcopy(s["lms"])
        if len(lms["status"]):
            po.estimate_depths(lms, texels, None, w.intr, T, s["e"], s["ab"], e_t, ab_t)
        want.append(lms)
    return pyr, Ts, want


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n_sets", [8, 9, 16])
def test_gpu_batched_estimate_matches_oracle(worlds, n_sets, dtype):
    """dsopp_hip_immature_sets_estimate with 8 (kernel-argument tables), 9 (first pinned-table call) and 16 sets (capacity):
    every set against the oracle and bitwise against its own per-set call; default streams, then one shared stream"""
    import ctypes
    from dsopp_amd import capi
    w = worlds(BATCH_SIZE)
    dt = capi.F64 if dtype == "f64" else capi.F32
    sets = _batch_sets(w, n_sets, seed=n_sets)
    T_w_t, e_t, ab_t = SCENARIOS["baseline"][1]
    pyr, Ts, want = _batch_oracle(w, sets, w.targets["baseline"][1], T_w_t, e_t, ab_t, dt)
    expo = np.array([s["e"] for s in sets])
    aff = np.array([s["ab"] for s in sets])
    single = []
    for s, T in zip(sets, Ts):
        d = capi.ImmatureSet(s["lms"])
        d.estimate(pyr, 0, w.intr, T, s["e"], s["ab"], e_t, ab_t)
        single.append(d.download())
        d.close()
    hip = ctypes.CDLL("libamdhip64.so")
    shared = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(shared)) == 0
    try:
        for stream in (None, shared.value):
            batch = [capi.ImmatureSet(s["lms"], stream=stream) for s in sets]
            capi.estimate_depths_batched(batch, pyr, 0, w.intr, Ts, expo, aff, e_t, ab_t)
            for k, (b, wnt, one) in enumerate(zip(batch, want, single)):
                got = b.download()
                _assert_parity(wnt, got, f"batch {n_sets} {dtype} set {k} stream {stream}")
                for f in got:
                    assert np.array_equal(got[f], one[f]), (k, f)
                b.close()
        assert sum(int((x["status"] == 0).sum()) for x in want) > 500
    finally:
        hip.hipStreamDestroy(shared)
        pyr.close()


@pytest.mark.gpu
@pytest.mark.parametrize("streams", ["shared", "own"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_gpu_batched_table_path_back_to_back(worlds, dtype, streams):
    """three pinned-table calls (16 sets) in a row on three different target pyramids, checked against the oracle applied in
    sequence.  shared: every set on one stream, so nothing synchronises the host between the calls: call k + 1 rewrites the lead
    set's pinned table while the copy of call k may still wait in the stream behind the launch of call k - 1, and only the
    tables_copied event orders the two.  own: a stream per set (the call then ends with a wait for the lead stream)"""
    import ctypes
    from dsopp_amd import capi
    from oracle import pyoracle as po
    w = worlds(BATCH_SIZE)
    dt = capi.F64 if dtype == "f64" else capi.F32
    sets = _batch_sets(w, 16, seed=99)
    targets = list(zip(SCENARIOS["baseline"], w.targets["baseline"]))
    pyrs = [_pyramid(w, u8, dt, None) for _, u8 in targets]
    want = [copy.deepcopy(s["lms"]) for s in sets]
    Ts_all = []
    for ((T_w_t, e_t, ab_t), _), pyr in zip(targets, pyrs):
        texels = pyr.get_level(0)
        Ts = np.stack([syn.mat_to_params(_inverse(T_w_t) @ s["T_w_r"]) for s in sets])
        Ts_all.append(Ts)
        for s, lms, T in zip(sets, want, Ts):
            if len(lms["status"]):
                po.estimate_depths(lms, texels, None, w.intr, T, s["e"], s["ab"], e_t, ab_t)
    expo = np.array([s["e"] for s in sets])
    aff = np.array([s["ab"] for s in sets])
    hip = ctypes.CDLL("libamdhip64.so")
    shared = ctypes.c_void_p()
    if streams == "shared":
        assert hip.hipStreamCreate(ctypes.byref(shared)) == 0
    batch = [capi.ImmatureSet(s["lms"], stream=shared.value) for s in sets]
    try:
        for ((T_w_t, e_t, ab_t), _), pyr, Ts in zip(targets, pyrs, Ts_all):
            capi.estimate_depths_batched(batch, pyr, 0, w.intr, Ts, expo, aff, e_t, ab_t)
        for k, (b, wnt) in enumerate(zip(batch, want)):
            _assert_parity(wnt, b.download(), f"back-to-back {dtype} {streams} streams, set {k}")
        assert sum(int((x["status"] == 0).sum()) for x in want) > 500
    finally:
        for b in batch:
            b.close()
        for p in pyrs:
            p.close()
        if shared.value:
            hip.hipStreamDestroy(shared)
