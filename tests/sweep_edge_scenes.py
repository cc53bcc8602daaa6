"""Windows that take the bundle-adjustment sweeps to the edges of their frames (no GPU needed to build them).

Every window has 3 keyframes and 240 landmarks (80 per keyframe), frame 0 fixed, the full clique of connections and synthetic.BASE_MOTION
poses with make_window's pose and inverse-depth noise: the smallest window in which all six directed pairs exist and the LM loop takes
more than one step.  What differs from synthetic.make_window is where the frames end and where the landmarks lie:

  interior(W, H)   make_window itself at a frame size that is no multiple of four (row stride and allocation of the tiled intensity plane)
  border(W, H)     integer landmarks in [2, W-3] x [2, H-3], about half of them within 8 pixels of an edge: the ROI decisions of the
                   reference side, of the target side and of the first-estimate-Jacobians item test all say "outside" somewhere
  mixed(sizes)     one 163 x 123 scene, every keyframe cropped at the origin to a size of its own (reference and target sizes differ)
  level(l)         327 x 245 8-bit frames through a photometric LUT and a 3-level pyramid, the window on level l (163 x 122, 81 x 61)
  masked_border()  border(161, 121) with a camera mask of a few rectangles per keyframe where landmarks reproject, and non-zero affine
                   brightness states

tests/test_sweep_edge_scenes.py asserts on the CPU oracle alone that the scenes reach what they are for; tests/test_gpu_sweep_frame_edges.py
compares the HIP window with the oracle on them; tests/test_gpu_sweep_f32.py compares its fp32 mode with tests/sweep_f32_model.py on
F32_EDGE_SCENES.  The builders are cached: the tests share one copy of every scene and leave it unchanged.
"""
import dataclasses
import functools

import numpy as np

from dsopp_amd import synthetic as syn

SIZES = [(161, 121), (162, 123), (163, 122), (160, 120)]   # W mod 4 = 1, 2, 3, 0; H mod 4 = 1, 3, 2, 0; both parities of H
ODD_SIZES = SIZES[:3]
MIXED_FULL = (163, 123)
MIXED_SIZES = ((163, 121), (160, 123), (162, 122))
MIXED_SIZES_PERMUTED = MIXED_SIZES[1:] + MIXED_SIZES[:1]     # every keyframe takes its successor's size
LEVEL_SIZE = (327, 245)                                      # -> 163 x 122 -> 81 x 61
LEVELS = 3
NUM_FRAMES, PER_FRAME = 3, 80
STATUS_OK, STATUS_OOB = 0, 3                                 # PointConnectionStatus of both backends
ROI_BORDER = 4                                               # inclusive ROI limits 4 and W - 5 (H - 5)


@dataclasses.dataclass
class EdgeScene:
    name: str
    window: syn.SyntheticWindow          # frames[i].pixelinfo is the image the window sees (the cropped plane / the pyramid level)
    intrinsics: np.ndarray               # of the window's level
    level: int = 0
    lut: np.ndarray = None               # level scenes: the HIP window builds its own pyramid of frames[i].image_u8 through this LUT
    masks: list = None                   # masked scenes: one H x W uint8 camera mask per keyframe (1 = valid, 0 = masked)

    def size(self, i):
        h, w = self.window.frames[i].pixelinfo.shape[:2]
        return w, h


def _poses(rng):
    """ground-truth and initial poses as synthetic.make_window draws them"""
    out = []
    for i in range(NUM_FRAMES):
        T_gt = syn.se3_exp(i * syn.BASE_MOTION)
        T_init = T_gt.copy()
        if i > 0:
            T_init = T_gt @ syn.se3_exp(np.concatenate([rng.normal(0, 2e-2, 3), rng.normal(0, 5e-3, 3)]))
        out.append((T_gt, T_init))
    return out


def _pick(rng, grad, n, x_lo, x_hi, y_lo, y_hi, min_gradient=4.0):
    """n distinct integer pixels of the inclusive box, those with |grad| > min_gradient first (make_window's landmark criterion)"""
    xs, ys = np.meshgrid(np.arange(x_lo, x_hi + 1), np.arange(y_lo, y_hi + 1))
    xs, ys = xs.ravel(), ys.ravel()
    perm = rng.permutation(len(xs))
    strong = grad[ys[perm], xs[perm]] > min_gradient
    perm = np.concatenate([perm[strong], perm[~strong]])[:n]
    assert len(perm) == n
    return np.stack([xs[perm], ys[perm]], axis=1).astype(np.float64)


def _frame(i, u8, pinfo, idepth_gt, poses, uv, rng, idepth_noise=2e-3):
    """a SyntheticFrame whose patches are read from the intensities the window samples"""
    ui, vi = uv[:, 0].astype(int), uv[:, 1].astype(int)
    idepth_init = idepth_gt * (1 + rng.uniform(-idepth_noise, idepth_noise, len(uv)))
    patch = np.stack([pinfo[vi + int(oy), ui + int(ox), 0] for ox, oy in syn.PATTERN], axis=1)
    T_gt, T_init = poses[i]
    return syn.SyntheticFrame(i, 1000 * (i + 1), u8, pinfo, None, T_gt, T_init, np.zeros(2), np.zeros(2), 1.0, i == 0, uv, idepth_gt,
                              idepth_init, patch)


def _render_u8(scene, T):
    img, depth = scene.render(T)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8), depth


@functools.lru_cache(maxsize=None)
def interior(width, height):
    win = syn.make_window(num_frames=NUM_FRAMES, num_points=NUM_FRAMES * PER_FRAME, width=width, height=height, seed=width + height)
    return EdgeScene(f"interior-{width}x{height}", win, win.scene.intrinsics)


# landmarks of a border keyframe, per edge: (count, nearest and farthest distance of the coordinate from that edge).  Distances 2 and 3:
# the pattern's centre itself is outside the ROI; 4 and 5: the centre is inside, the pattern's arm (u +- 2) is not; 6 and 7: the reference
# side is inside and the target side decides; 8 .. 13: inside, and the reprojection stays within 8 pixels of the target's limit.
BORDER_BANDS = ((3, 2, 3), (2, 4, 5), (6, 6, 7), (4, 8, 13))
BORDER_UNIFORM = PER_FRAME - 4 * sum(b[0] for b in BORDER_BANDS)   # the rest: anywhere in [8, W-9] x [8, H-9]


@functools.lru_cache(maxsize=None)
def border(width, height):
    scene = syn.Scene.make(width, height, seed=1000 + width + height)
    rng = np.random.default_rng(2000 + width + height)
    poses = _poses(rng)
    frames = []
    for i in range(NUM_FRAMES):
        u8, depth = _render_u8(scene, poses[i][0])
        pinfo = syn.pixelinfo_from_plane(u8.astype(np.float64))
        grad = np.hypot(pinfo[..., 1], pinfo[..., 2])
        parts = []
        for count, near, far in BORDER_BANDS:
            # along the edge: anywhere the patch can be read for the outermost band (corners included), clear of the other edges otherwise
            a = 2 if near < 4 else 8
            parts += [_pick(rng, grad, count, near, far, a, height - 1 - a),                              # left
                      _pick(rng, grad, count, width - 1 - far, width - 1 - near, a, height - 1 - a),      # right
                      _pick(rng, grad, count, a, width - 1 - a, near, far),                               # top
                      _pick(rng, grad, count, a, width - 1 - a, height - 1 - far, height - 1 - near)]     # bottom
        parts.append(_pick(rng, grad, BORDER_UNIFORM, 8, width - 9, 8, height - 9))
        uv = np.concatenate(parts)
        uv = uv[rng.permutation(len(uv))]
        assert len(uv) == PER_FRAME
        frames.append(_frame(i, u8, pinfo, 1.0 / depth[uv[:, 1].astype(int), uv[:, 0].astype(int)], poses, uv, rng))
    return EdgeScene(f"border-{width}x{height}", syn.SyntheticWindow(scene, frames), scene.intrinsics)


@functools.lru_cache(maxsize=None)
def _mixed_base():
    """renders, poses and landmarks of the mixed scene: the landmarks are interior to the keyframes' MIXED_SIZES"""
    scene = syn.Scene.make(*MIXED_FULL, seed=77)
    rng = np.random.default_rng(78)
    poses = _poses(rng)
    base = []
    for i, (w, h) in enumerate(MIXED_SIZES):
        u8, depth = _render_u8(scene, poses[i][0])
        pinfo = syn.pixelinfo_from_plane(u8[:h, :w].astype(np.float64))
        uv = _pick(rng, np.hypot(pinfo[..., 1], pinfo[..., 2]), PER_FRAME, 8, w - 9, 8, h - 9)
        f = _frame(i, u8, pinfo, 1.0 / depth[uv[:, 1].astype(int), uv[:, 0].astype(int)], poses, uv, rng)
        base.append(f)
    return scene, base


@functools.lru_cache(maxsize=None)
def mixed(sizes=MIXED_SIZES):
    """the mixed window with keyframe i cropped (at the origin: same intrinsics, still photoconsistent) to sizes[i].  Poses, landmarks,
    patches and inverse depths do not depend on `sizes`: two windows differ in nothing but where their frames end."""
    scene, base = _mixed_base()
    frames = []
    for f, (w, h) in zip(base, sizes):
        assert f.uv[:, 0].max() <= w - 3 and f.uv[:, 1].max() <= h - 3          # the patch still lies in the frame
        u8 = np.ascontiguousarray(f.image_u8[:h, :w])
        frames.append(dataclasses.replace(f, image_u8=u8, pixelinfo=syn.pixelinfo_from_plane(u8.astype(np.float64))))
    return EdgeScene("mixed-" + "-".join(f"{w}x{h}" for w, h in sizes), syn.SyntheticWindow(scene, frames), scene.intrinsics)


@functools.lru_cache(maxsize=None)
def _level_base():
    from oracle import pyoracle as po
    scene = syn.Scene.make(*LEVEL_SIZE, seed=91)
    rng = np.random.default_rng(92)
    lut = np.cumsum(rng.uniform(0.5, 1.5, 256))       # monotone, and no round numbers: the intensities use their whole mantissa
    poses = _poses(rng)
    frames = []
    for i in range(NUM_FRAMES):
        u8, depth = _render_u8(scene, poses[i][0])
        frames.append((u8, depth, po.build_pyramid(u8, lut=lut, levels=LEVELS)[0]))
    return scene, lut, poses, frames


@functools.lru_cache(maxsize=None)
def level(l):
    """the window on pyramid level l: landmarks are integer pixels of that level, inverse depths those of the level-0 pixel (u << l, v << l),
    intrinsics divided by 1 << l (CameraCalibration::cameraModel(level))"""
    scene, lut, poses, base = _level_base()
    rng = np.random.default_rng(93 + l)
    frames = []
    for i, (u8, depth, infos) in enumerate(base):
        pinfo = infos[l]
        h, w = pinfo.shape[:2]
        assert (w, h) == (LEVEL_SIZE[0] >> l, LEVEL_SIZE[1] >> l)
        uv = _pick(rng, np.hypot(pinfo[..., 1], pinfo[..., 2]), PER_FRAME, 8, w - 9, 8, h - 9)
        idepth_gt = 1.0 / depth[uv[:, 1].astype(int) << l, uv[:, 0].astype(int) << l]
        frames.append(_frame(i, u8, pinfo, idepth_gt, poses, uv, rng))
    return EdgeScene(f"level{l}", syn.SyntheticWindow(scene, frames), scene.intrinsics / (1 << l), level=l, lut=lut)


# (name, builder) of every scene of the f64 comparisons, and of the f32 ones (no border scene there: fp32 reprojection legitimately flips
# ROI decisions that sit on the limit)
F64_SCENES = ([(f"interior-{w}x{h}", functools.partial(interior, w, h)) for w, h in SIZES]
              + [(f"border-{w}x{h}", functools.partial(border, w, h)) for w, h in SIZES]
              + [("mixed", mixed), ("level1", functools.partial(level, 1)), ("level2", functools.partial(level, 2))])
F32_SCENES = ([(f"interior-{w}x{h}", functools.partial(interior, w, h)) for w, h in ODD_SIZES]
              + [("mixed", mixed), ("level1", functools.partial(level, 1))])


MASK_RECTS, MASK_RECT_W, MASK_RECT_H = 5, 7, 5
MASKED_AFFINE = ((0.0, 0.0), (0.02, 1.5), (-0.03, -2.5))     # (a, b) of the masked scene's keyframes: b_t, b_r and s are no longer 0, 0, 1


@functools.lru_cache(maxsize=None)
def masked_border(width=SIZES[0][0], height=SIZES[0][1]):
    """border(width, height) whose keyframes carry a camera mask: MASK_RECTS rectangles of MASK_RECT_W x MASK_RECT_H masked pixels per
    keyframe, each with a corner one pixel beside the reprojection of a landmark of another keyframe, so that patterns lie across a
    mask edge (some of their 8 pixels masked, some not) as well as wholly inside and outside one.  The keyframes also start from the
    affine brightness states MASKED_AFFINE: every other scene has a = b = 0, where a residual without its b_t is the same residual."""
    base = border(width, height)
    rng = np.random.default_rng(3000 + width + height)
    frames = [dataclasses.replace(f, affine_init=np.array(MASKED_AFFINE[i])) for i, f in enumerate(base.window.frames)]
    scene = EdgeScene(f"masked-border-{width}x{height}", syn.SyntheticWindow(base.window.scene, frames), base.intrinsics)
    masks = []
    for t in range(NUM_FRAMES):
        mask = np.ones((height, width), dtype=np.uint8)
        centres = []
        for r in range(NUM_FRAMES):
            if r != t:
                tu, tv = reproject_centres(scene, r, t)
                inside = (tu >= 12) & (tu <= width - 13) & (tv >= 12) & (tv <= height - 13)
                centres.append(np.stack([tu[inside], tv[inside]], axis=1))
        centres = np.concatenate(centres)
        for cu, cv in centres[rng.choice(len(centres), MASK_RECTS, replace=False)]:
            x0, y0 = int(np.rint(cu)) + 1, int(np.rint(cv)) - MASK_RECT_H // 2
            mask[y0:y0 + MASK_RECT_H, x0:x0 + MASK_RECT_W] = 0
        masks.append(mask)
    scene.masks = masks
    return scene


# the scenes of the residual-by-residual f32 comparison (tests/sweep_f32_model.py judges every ROI decision by its margin, so the border
# scenes are in): every size of the interior and border scenes, the mixed one, both levels and the masked border scene
F32_EDGE_SCENES = ([(f"interior-{w}x{h}", functools.partial(interior, w, h)) for w, h in SIZES]
                   + [(f"border-{w}x{h}", functools.partial(border, w, h)) for w, h in SIZES]
                   + [("mixed", mixed), ("level1", functools.partial(level, 1)), ("level2", functools.partial(level, 2)),
                      ("masked-border", masked_border)])


def load(backend, scene, pyramids=None):
    """synthetic.load_window for an EdgeScene.  `pyramids`: one device pyramid per keyframe for the HIP window to borrow at scene.level
    (build_pyramids); without them the backend is handed frames[i].pixelinfo, which is what the oracle always takes.  A scene's camera
    masks go with the pixelinfo (push_frame's mask argument); no scene has both masks and borrowed pyramids."""
    win = scene.window
    assert scene.masks is None or pyramids is None
    for i, f in enumerate(win.frames):
        mask = None if scene.masks is None else scene.masks[i]
        args = (f.frame_id, f.timestamp, f.pixelinfo, mask, scene.intrinsics, syn.mat_to_params(f.T_w_c_init), f.exposure, f.affine_init,
                f.fixed, False)
        if pyramids is None:
            backend.push_frame(*args)
        else:
            backend.push_frame(*args, pyramid=pyramids[i], level=scene.level)
        backend.set_landmarks(f.frame_id, f.uv, f.idepth_init, f.patch, np.zeros(len(f.uv), dtype=np.uint8))
        for j in range(i):
            g = win.frames[j]
            for r, t in ((g, f), (f, g)):
                backend.set_connection(r.frame_id, t.frame_id, np.zeros(len(r.uv), dtype=np.uint8))
    return backend


def build_pyramids(scene, dtype):
    """device pyramids of a level scene's 8-bit frames, built through its LUT (None for the scenes that hand pixelinfo over)"""
    if scene.lut is None:
        return None
    from dsopp_amd import capi
    out = []
    for f in scene.window.frames:
        p = capi.Pyramid(LEVEL_SIZE[0], LEVEL_SIZE[1], LEVELS, dtype=dtype)
        p.build(f.image_u8, lut=scene.lut)
        out.append(p)
    return out


def pairs(scene):
    ids = [f.frame_id for f in scene.window.frames]
    return [(r, t) for r in ids for t in ids if r != t]


def reproject_centres(scene, r, t):
    """(tu, tv) of the landmarks of keyframe r in keyframe t from the initial poses and inverse depths, in plain numpy"""
    fr, ft = scene.window.frames[r], scene.window.frames[t]
    fx, fy, cx, cy = scene.intrinsics
    T = np.linalg.inv(ft.T_w_c_init) @ fr.T_w_c_init
    rays = np.stack([(fr.uv[:, 0] - cx) / fx, (fr.uv[:, 1] - cy) / fy, np.ones(len(fr.uv))], axis=0)
    p = T[:3, :3] @ rays + T[:3, 3:4] * fr.idepth_init[None, :]
    return fx * p[0] / p[2] + cx, fy * p[1] / p[2] + cy
