"""NumPy statement of the tracker's two debug views (include/dsopp_hip.h, "the tracker's debug views"; dsopp_amd/csrc/debug_views.hip):
the frame view, the keyframe view's average in the kernel's stated summation order, the state M, the levels, and two renderers of the
keyframe view — the GATHER the device runs (a pixel takes the occupied stencil tap with the largest (y, x)) and an independent PAINTER
that follows the reference literally (raster-order loops, stamp the footprint, later over earlier).  tests/test_debug_views_model.py
holds the two against each other; tests/test_gpu_debug_views.py holds the kernels to this file byte for byte and M bit for bit."""
import numpy as np

RADIUS, SIDE = 3, 7
EMPTY = -1
BLOCK, CHUNK = 256, 4096


def default_stencil():
    """dx^2 + dy^2 <= 9 as 7 x 7 bytes, index (dy + 3, dx + 3)"""
    d = np.arange(-RADIUS, RADIUS + 1)
    return (d[:, None] ** 2 + d[None, :] ** 2 <= RADIUS * RADIUS).astype(np.uint8)


def default_colormap():
    """the library's jet as 256 x {B, G, R}: x = v / 255, channel = rint(255 clamp(1.5 - |4 x - centre|, 0, 1)), centres 1 (B), 2 (G), 3 (R)"""
    x = np.arange(256) / 255.0
    return np.stack([np.rint(255.0 * np.clip(1.5 - np.abs(4.0 * x - centre), 0.0, 1.0)) for centre in (1.0, 2.0, 3.0)], axis=1).astype(np.uint8)


def frame_view(grey, mask=None):
    """(H, W) grey bytes and mask bytes (None = all valid; 0 = masked) -> (H, W, 3) BGR"""
    g = np.asarray(grey, dtype=np.uint8)
    out = np.repeat(g[..., None], 3, axis=2)
    if mask is not None:
        m = np.asarray(mask) == 0
        dark = np.maximum(g.astype(np.int32) - 128, 0).astype(np.uint8)
        out[..., 0] = np.where(m, dark, g)
        out[..., 1] = np.where(m, dark, g)
    return out


def quotients(ids, wgt):
    """(qualifies, q) per cell in row-major order; q = 0.0 where the cell does not qualify"""
    ids, wgt = np.asarray(ids, dtype=np.float64).reshape(-1), np.asarray(wgt, dtype=np.float64).reshape(-1)
    ok = ids > 0
    q = np.zeros(ids.shape)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        q[ok] = ids[ok] / wgt[ok]
    return ok, q


def _waves(s):
    """(..., 256) per-thread sums -> (...,): every wave's 64 lanes by the shuffle tree, then the four waves in order"""
    v = s.reshape(s.shape[:-1] + (BLOCK // 64, 64)).copy()
    off = 32
    while off:
        v[..., :off] = v[..., :off] + v[..., off:2 * off]
        off //= 2
    w = v[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def stated_sum(q):
    """the sum of q in the order the header states (chunks of 4096, sixteen per thread, waves, then the chunks' sums the same way)"""
    with np.errstate(invalid="ignore", over="ignore"):
        blocks = -(-len(q) // CHUNK)
        padded = np.zeros(blocks * CHUNK)
        padded[:len(q)] = q
        c = padded.reshape(blocks, CHUNK // BLOCK, BLOCK)
        s = np.zeros((blocks, BLOCK))
        for k in range(CHUNK // BLOCK):
            s = s + c[:, k]
        partial = _waves(s)
        rounds = -(-blocks // BLOCK)
        p = np.zeros(rounds * BLOCK)
        p[:blocks] = partial
        t = np.zeros(BLOCK)
        for r in range(rounds):
            t = t + p[r * BLOCK:(r + 1) * BLOCK]
        return float(_waves(t))


def serial_sum(q):
    """the plain raster-order sum, one addition per qualifying cell, as std::accumulate takes it"""
    s = 0.0
    for v in q:
        s += v
    return s


def update_state(M, total, cells):
    """step 2: the new M (unchanged without a cell)"""
    if cells == 0:
        return M
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        avg = np.float64(total) / np.float64(cells)
        twice = np.float64(2.0) * avg
        M = np.float64(M)
        if M == 0:
            M = twice
        return float(np.float64(0.9) * M + np.float64(0.1) * twice)


def unrounded_levels(ids, wgt, M):
    """(255 q) / M per cell before clamp and rint (NaN where the cell does not qualify is NOT used: see levels)"""
    ok, q = quotients(ids, wgt)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return ok, (255.0 * q) / np.float64(M)


def levels(ids, wgt, M):
    """(H, W) int: EMPTY where the cell does not qualify, else rint(clamp((255 q) / M, 0, 255)), half to even, NaN -> 0"""
    shape = np.asarray(ids).shape
    ok, v = unrounded_levels(ids, wgt, M)
    v = np.where(v >= 0.0, v, 0.0)       # below 0, and NaN
    v = np.where(v > 255.0, 255.0, v)
    out = np.rint(v).astype(np.int64)
    out[~ok] = EMPTY
    return out.reshape(shape)


def render_painter(grey, lv, colormap=None, stencil=None):
    """the reference, literally: cells in raster order (y outer, x inner), each stamps its footprint, clipped; later overwrites earlier"""
    colormap = default_colormap() if colormap is None else np.asarray(colormap, dtype=np.uint8).reshape(256, 3)
    stencil = default_stencil() if stencil is None else np.asarray(stencil).reshape(SIDE, SIDE)
    H, W = lv.shape
    painted = np.full((H, W), EMPTY, dtype=np.int64)
    offsets = [(dy - RADIUS, dx - RADIUS) for dy in range(SIDE) for dx in range(SIDE) if stencil[dy, dx]]
    ys, xs = np.nonzero(lv != EMPTY)             # (np.nonzero walks in row-major order: y outer, x inner)
    for y, x in zip(ys.tolist(), xs.tolist()):
        level = lv[y, x]
        for dy, dx in offsets:
            py, px = y + dy, x + dx
            if 0 <= py < H and 0 <= px < W:
                painted[py, px] = level
    out = np.repeat(np.asarray(grey, dtype=np.uint8)[..., None], 3, axis=2)
    covered = painted != EMPTY
    out[covered] = colormap[painted[covered]]
    return out


def render_gather(grey, lv, colormap=None, stencil=None):
    """what the device does: pixel p scans the set taps c = p - (dx, dy) in ascending (dy, dx) — descending (c.y, c.x) — and takes the
    first occupied cell"""
    colormap = default_colormap() if colormap is None else np.asarray(colormap, dtype=np.uint8).reshape(256, 3)
    stencil = default_stencil() if stencil is None else np.asarray(stencil).reshape(SIDE, SIDE)
    H, W = lv.shape
    padded = np.full((H + 2 * RADIUS, W + 2 * RADIUS), EMPTY, dtype=np.int64)
    padded[RADIUS:RADIUS + H, RADIUS:RADIUS + W] = lv
    winner = np.full((H, W), EMPTY, dtype=np.int64)
    for sy in range(SIDE):
        for sx in range(SIDE):
            if not stencil[sy, sx]:
                continue
            dy, dx = sy - RADIUS, sx - RADIUS
            tap = padded[RADIUS - dy:RADIUS - dy + H, RADIUS - dx:RADIUS - dx + W]    # the cell p - (dx, dy) for every p
            winner = np.where((winner == EMPTY) & (tap != EMPTY), tap, winner)
    out = np.repeat(np.asarray(grey, dtype=np.uint8)[..., None], 3, axis=2)
    covered = winner != EMPTY
    out[covered] = colormap[winner[covered]]
    return out


def keyframe_view(grey, ids, wgt, M, colormap=None, stencil=None, render=render_gather):
    """-> (BGR image, the new M, cells)"""
    ok, q = quotients(ids, wgt)
    cells = int(ok.sum())
    M = update_state(M, stated_sum(q), cells)
    lv = levels(ids, wgt, M) if cells else np.full(np.asarray(ids).shape, EMPTY, dtype=np.int64)
    return render(grey, lv, colormap, stencil), M, cells


# ---- the cases both test files run: exact planes on every decision edge, then seeded random ones

def grey_image(W, H, seed=0):
    """random bytes with 0, 127, 128 and 255 certainly among them"""
    g = np.random.default_rng(1000 + 31 * W + H + seed).integers(0, 256, (H, W)).astype(np.uint8)
    g.reshape(-1)[:4] = (0, 127, 128, 255)
    return g


def _planes(W, H, cells, weight=0.5):
    """cells: (x, y, q) with dyadic q: idepth_sum = q * weight exactly, so the division gives q back exactly"""
    ids, wgt = np.zeros((H, W)), np.zeros((H, W))
    for x, y, q in cells:
        ids[y, x], wgt[y, x] = q * weight, weight
    return ids, wgt


def _clipping():
    """61 x 47: a cell at each corner, at each edge midpoint, and at distances 1, 2 and 3 from each edge"""
    W, H = 61, 47
    at = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, 0), (W // 2, H - 1), (0, H // 2), (W - 1, H // 2)]
    for d in (1, 2, 3):
        at += [(d, 3 + 9 * d), (W - 1 - d, 3 + 9 * d), (8 + 9 * d, d), (8 + 9 * d, H - 1 - d)]
    return dict(W=W, H=H, planes=_planes(W, H, [(x, y, (1 + i) / 16.0) for i, (x, y) in enumerate(at)]), cells=len(at))


def _pairs():
    """230 x 200: every arrangement (dx, dy) in [-6, 6]^2 without the origin of two cells with different levels, on a 16-pixel grid"""
    W, H = 230, 200
    arrangements = [(dx, dy) for dy in range(-6, 7) for dx in range(-6, 7) if (dx, dy) != (0, 0)]
    assert len(arrangements) == 14 * 12
    cells = []
    for i, (dx, dy) in enumerate(arrangements):
        cx, cy = 8 + 16 * (i % 14), 8 + 16 * (i // 14)
        cells += [(cx, cy, 0.25), (cx + dx, cy + dy, 1.5)]
    return dict(W=W, H=H, planes=_planes(W, H, cells), cells=len(cells))


TIE_LEVELS = (0, 1, 2, 3, 10, 11, 100, 101, 253, 254)


def _ties():
    """40 x 30, from M = 0: ten cells q = (k + 1/2) / 64 and one that makes the average 255 / 128 exactly, so that M = 255 / 64 and the
    unrounded levels are k + 1/2 exactly (the tests assert it from the model); the eleventh cell lies above M: level 255"""
    W, H = 40, 30
    q = [(k + 0.5) / 64.0 for k in TIE_LEVELS]
    q.append(11 * 255.0 / 128.0 - sum(q))
    return dict(W=W, H=H, planes=_planes(W, H, [(4 + 9 * (i % 4), 3 + 8 * (i // 4), v) for i, v in enumerate(q)]), cells=11)


def _range():
    """33 x 21: one huge q sets M (level 255 for itself), a tiny q and a negative q (negative weight) give level 0; four cells that do not
    qualify: idepth -1, 0 with weight 1, 0 with weight 0, -0.0"""
    W, H = 33, 21
    ids, wgt = _planes(W, H, [(5, 5, 2.0 ** 20), (15, 5, 2.0 ** -1000), (25, 5, 1.0)])
    ids[15, 5], wgt[15, 5] = 1.0, -4.0
    for x, (i, w) in zip((12, 17, 22, 27), ((-1.0, 1.0), (0.0, 1.0), (0.0, 0.0), (-0.0, 2.0))):
        ids[15, x], wgt[15, x] = i, w
    return dict(W=W, H=H, planes=(ids, wgt), cells=4)


def _random(W, H, occupancy, seed):
    rng = np.random.default_rng(seed)
    on = rng.random((H, W)) < occupancy
    wgt = np.where(on, rng.uniform(0.5, 2.0, (H, W)), 0.0)
    ids = np.where(on, rng.uniform(0.1, 3.0, (H, W)) * wgt, 0.0)
    return dict(W=W, H=H, planes=(ids, wgt), cells=int(on.sum()), random=True)


EXACT_CASES = {"clipping": _clipping, "pairs": _pairs, "ties": _ties, "range": _range}
RANDOM_CASES = {f"{W}x{H}_{int(100 * occ)}pct": (lambda W=W, H=H, occ=occ, k=k: _random(W, H, occ, 50 + k))
                for k, (W, H, occ) in enumerate((W, H, occ) for (W, H) in ((300, 41), (24, 4120), (360, 280)) for occ in (0.01, 0.5))}
# 257 chunks of 4096 cells: the closing workgroup's second round (a 1280 x 1024 map has 320)
RANDOM_CASES["1042x1009_1pct"] = lambda: _random(1042, 1009, 0.01, 60)
CASES = dict(EXACT_CASES, **RANDOM_CASES)

_cache = {}


def case(name):
    """computed once, shared by the tests, never written to"""
    if name not in _cache:
        c = CASES[name]()
        c["name"] = name
        c["grey"] = grey_image(c["W"], c["H"])
        for a in c["planes"] + (c["grey"],):
            a.setflags(write=False)
        _cache[name] = c
    return _cache[name]


def custom_colormap():
    """a table no channel of which repeats the library's: B = v, G = 255 - v, R = 37 v mod 256"""
    v = np.arange(256)
    return np.stack([v, 255 - v, (37 * v) % 256], axis=1).astype(np.uint8)


def asymmetric_stencil():
    """the centre, an arm of 3 to the right (+dx), an arm of 2 down (+dy) and one pixel up-left: no symmetry of the square keeps it"""
    s = np.zeros((SIDE, SIDE), dtype=np.uint8)
    s[RADIUS, RADIUS:RADIUS + 4] = 1
    s[RADIUS:RADIUS + 3, RADIUS] = 1
    s[RADIUS - 1, RADIUS - 2] = 1
    return s
