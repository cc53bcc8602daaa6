"""NumPy restatement of the reference's `eigen` tracking-feature extractor (DSO's pixel selector,
src/features/src/eigen_tracking_features_extractor.cpp), the test side of dsopp_amd/csrc/features_eigen.hip:

  1. the extractor's own pyramid: 5 levels of the u8 image with an identity LUT and no vignette (the tracker's pyramid rule,
     dsopp_hip_pyramid_build with lut256 = vignetting = NULL; here from the CPU oracle, which test_gpu_tracker.py holds bit-exact);
  2. random pattern: srand(3141592), then W * H bytes (uint8_t)rand() of glibc's TYPE_3 generator;
  3. 16 directions (cos, sin) from Taylor polynomials (degree 8 / 9) at -pi/2 + (pi/16) i, evaluated as written;
  4. the camera mask eroded by 15 x 15 (features_model.eroded_valid);
  5. threshold map: (W/32) x (H/32) cells; per cell the histogram of (int)min(|g|, 49) over the valid pixels of
     [max(cw i, 1), min(cw (i+1), W-2)) x (the same in y), its median bin (first bin where the running sum passes round(total / 2),
     else 0) + 7, then the square of the mean over the 3 x 3 neighbourhood clipped to the map;
  6. findBestCandidate for a visited level-0 pixel (x, y): border 4 <= x < W-5, 4 <= y <= H-5, the map cell (x>>5, y>>5) inside the
     map; per level l the threshold is multiplied by 0.75^l (cumulative), a level whose candidate is -2 is skipped, x>>l < 4 or
     y>>l < 4 ends the pixel; accept when g^2 > thr and |cos dx + sin dy| > weight_l (each product and the sum rounded):
     weight_l = g^2, cand_l = (x, y), every level above becomes -2;
  7. windows: a level-L window (2^L p wide) visits its 2 x 2 children (a level-0 window its p x p pixels) in row-major order,
     skipping a child whose corner fails the eroded mask (outside the image included); before each child dir_L = directions[
     pattern[n] & 15] with n the number of features emitted so far; at the end a candidate with x > 0 is emitted and
     weight_{L+1} = 1e10; top windows are level 4, stepping 16 p over the image in row-major order;
  8. potential control: ratio = desired / found; ideal = max(1, (int)(sqrt(1 / ratio) (p + 1) - 1)); ratio > 1.25 and p > 1: p =
     min(ideal, p - 1) and a second pass; else ratio < 0.25: p = max(ideal, p + 1) and a second pass; at most two passes; after
     the last, ratio < 0.95 keeps the features with pattern[x + y W] <= (int)(255 ratio), in order.  p starts at 15 and persists.

The walk of rules 6-7 is written twice: `walk_literal` calls find_best_candidate for every visited pixel exactly as the reference
does (small images only); `walk` gives the same list faster by evaluating a level-0 window's pixels together (within one level-0
window n, and so every direction, is constant) and by skipping regions where no pixel passes the direction-free part of rule 6.
`ParallelPrototype` is the order-free formulation the device runs (see its docstring)."""
import functools
import math

import numpy as np

import features_model as fm

LEVELS = 5
BORDER = 4
INITIAL_POTENTIAL = 15
SEED = 3141592
MAX_GRADIENT_BINS = 50
MIN_GRADIENT = 7.0
DOWNWEIGHT = 0.75
BLOCKED = -2   # cand_l = (-2, -2)
NONE = -1      # cand_l = (-1, -1)


@functools.lru_cache(maxsize=None)
def _glibc_rand_bytes(n, seed=SEED):
    """(uint8_t)rand() n times after srand(seed): glibc's TYPE_3 additive feedback generator (degree 31, separation 3)"""
    r = [0] * 34
    r[0] = seed if seed != 0 else 1
    for i in range(1, 31):
        hi, lo = divmod(r[i - 1], 127773)
        word = 16807 * lo - 2836 * hi
        if word < 0:
            word += 2147483647
        r[i] = word
    state = r[:31]             # the 31 words after seeding; rand() adds the rear word (index b) into the front word (index f)
    out = bytearray(n)
    f, b = 3, 0
    for _ in range(310):       # srand discards 10 * 31 outputs
        state[f] = (state[f] + state[b]) & 0xFFFFFFFF
        f = 0 if f == 30 else f + 1
        b = 0 if b == 30 else b + 1
    for k in range(n):
        state[f] = (state[f] + state[b]) & 0xFFFFFFFF
        out[k] = (state[f] >> 1) & 0xFF
        f = 0 if f == 30 else f + 1
        b = 0 if b == 30 else b + 1
    return bytes(out)


def random_pattern(n):
    """rule 2: n bytes as uint8"""
    return np.frombuffer(_glibc_rand_bytes(int(n)), dtype=np.uint8)


def directions():
    """rule 3: (16, 2) float64 (cos, sin), each term as the reference writes it, left to right"""
    out = np.zeros((16, 2))
    for i in range(16):
        a = -math.pi / 2 + (math.pi / 16) * float(i)
        c = (1 - a * a / (1 * 2) + a * a * a * a / (1 * 2 * 3 * 4) - a * a * a * a * a * a / (1 * 2 * 3 * 4 * 5 * 6)
             + a * a * a * a * a * a * a * a / (1 * 2 * 3 * 4 * 5 * 6 * 7 * 8))
        s = (a - a * a * a / (1 * 2 * 3) + a * a * a * a * a / (1 * 2 * 3 * 4 * 5) - a * a * a * a * a * a * a / (1 * 2 * 3 * 4 * 5 * 6 * 7)
             + a * a * a * a * a * a * a * a * a / (1 * 2 * 3 * 4 * 5 * 6 * 7 * 8 * 9))
        out[i] = (c, s)
    return out


DIRECTIONS = directions()


def level_factor(level):
    """pow(0.75, level) as the reference's loop computes it"""
    r = 1.0
    for _ in range(level):
        r *= DOWNWEIGHT
    return r


def _median_bin(hist):
    thr = int(math.floor(float(int(hist.sum())) * 0.5 + 0.5))   # std::round of a non-negative x.0 / x.5
    for i, v in enumerate(hist):
        thr -= int(v)
        if thr < 0:
            return i
    return 0


def threshold_map(dx, dy, valid):
    """rule 5: (H/32, W/32) float64 from level-0 gradients (H x W) and the eroded mask"""
    H, W = dx.shape
    mw, mh = W // 32, H // 32
    cw, ch = W // mw, H // mh
    raw = np.zeros((mh, mw))
    g = np.minimum(np.sqrt(dx * dx + dy * dy), float(MAX_GRADIENT_BINS - 1)).astype(np.int64)
    for j in range(mh):
        y0, y1 = max(ch * j, 1), min(ch * (j + 1), H - 2)
        for i in range(mw):
            x0, x1 = max(cw * i, 1), min(cw * (i + 1), W - 2)
            hist = np.zeros(MAX_GRADIENT_BINS, dtype=np.int64)
            if y1 > y0 and x1 > x0:
                sel = g[y0:y1, x0:x1][valid[y0:y1, x0:x1]]
                hist = np.bincount(sel, minlength=MAX_GRADIENT_BINS)
            raw[j, i] = float(_median_bin(hist)) + MIN_GRADIENT
    out = np.zeros_like(raw)
    for j in range(mh):
        for i in range(mw):
            s, k = 0.0, 0.0
            for a in (-1, 0, 1):          # x outer, y inner as the reference sums
                for b in (-1, 0, 1):
                    if 0 <= i + a < mw and 0 <= j + b < mh:
                        k += 1.0
                        s += raw[j + b, i + a]
            out[j, i] = (s / k) * (s / k)
    return out


class Fields:
    """the per-pixel, direction-free part of rule 6 over level 0: A[l] (H x W bool) = the pixel passes the border, map and
    g^2 > thr_l tests of level l (and of every level below it: the pixel's processing ends at the first failing border);
    DX[l], DY[l], G2[l] = level l's gradient at (x >> l, y >> l)"""

    def __init__(self, infos, tmap, valid):
        H, W = infos[0].shape[:2]
        self.W, self.H, self.valid, self.infos, self.tmap = W, H, valid, infos, tmap
        ys, xs = np.mgrid[0:H, 0:W]
        mh, mw = tmap.shape
        ok = (xs >= BORDER) & (xs < W - 1 - BORDER) & (ys >= BORDER) & (ys <= H - 1 - BORDER) & ((xs >> 5) < mw) & ((ys >> 5) < mh)
        thr = tmap[np.minimum(ys >> 5, mh - 1), np.minimum(xs >> 5, mw - 1)]
        self.A, self.DX, self.DY, self.G2 = [], [], [], []
        for l in range(LEVELS):
            thr = thr * level_factor(l)
            xl, yl = xs >> l, ys >> l
            ok = ok & (xl >= BORDER) & (xl < W - 1 - BORDER) & (yl >= BORDER) & (yl <= H - 1 - BORDER)
            h, w = infos[l].shape[:2]
            t = infos[l][np.minimum(yl, h - 1), np.minimum(xl, w - 1)]
            dx, dy = t[..., 1].copy(), t[..., 2].copy()
            g2 = dx * dx + dy * dy
            self.A.append(ok & (g2 > thr))
            self.DX.append(dx)
            self.DY.append(dy)
            self.G2.append(g2)
        self.any = np.zeros((H, W), dtype=bool)
        for a in self.A:
            self.any |= a
        self.sat = np.zeros((H + 1, W + 1), dtype=np.int64)   # summed-area table of `any` (region skipping)
        self.sat[1:, 1:] = np.cumsum(np.cumsum(self.any, axis=0), axis=1)

    def region_has_any(self, x0, y0, w):
        x1, y1 = min(x0 + w, self.W), min(y0 + w, self.H)
        if x1 <= x0 or y1 <= y0:
            return False
        s = self.sat
        return s[y1, x1] - s[y0, x1] - s[y1, x0] + s[y0, x0] > 0

    def visited(self, x, y):
        """CameraMask::valid of the eroded mask: false outside the image"""
        return 0 <= x < self.W and 0 <= y < self.H and bool(self.valid[y, x])


def projection(c, s, dx, dy):
    """|cos dx + sin dy| with each product and the sum rounded (no fused multiply-add)"""
    return np.abs(np.float64(c) * dx + np.float64(s) * dy)


class _Walker:
    """rules 6-7 over one pass: the state the reference keeps in candidate_coords / candidate_weight / random_direction"""

    def __init__(self, F, p, pattern, literal=False):
        self.F, self.p, self.pattern, self.literal = F, p, pattern, literal
        self.cand = [NONE] * LEVELS    # NONE, BLOCKED or the pixel index y * W + x
        self.weight = [0.0] * LEVELS
        self.dir = [(0.0, 0.0)] * LEVELS
        self.features = []             # (pixel index, level) in emission order

    def set_dir(self, level):
        n = len(self.features)
        self.dir[level] = tuple(DIRECTIONS[int(self.pattern[n]) & 15])

    def best_candidate(self, x, y):
        """findBestCandidate for one pixel, literally"""
        F, W, H = self.F, self.F.W, self.F.H
        if x < BORDER or x >= W - 1 - BORDER or y < BORDER or y > H - 1 - BORDER:
            return
        xi, yj = x >> 5, y >> 5
        if xi >= F.tmap.shape[1] or yj >= F.tmap.shape[0]:
            return
        thr = float(F.tmap[yj, xi])
        for l in range(LEVELS):
            thr = thr * level_factor(l)
            if self.cand[l] == BLOCKED:
                continue
            xl, yl = x >> l, y >> l
            if xl < BORDER or xl >= W - 1 - BORDER or yl < BORDER or yl > H - 1 - BORDER:
                return
            dx, dy = float(F.infos[l][yl, xl, 1]), float(F.infos[l][yl, xl, 2])
            g2 = dx * dx + dy * dy
            c, s = self.dir[l]
            pr = abs(c * dx + s * dy)
            if g2 > thr and pr > self.weight[l]:
                self.weight[l] = g2
                self.cand[l] = y * W + x
                for k in range(l + 1, LEVELS):
                    self.cand[k] = BLOCKED

    def level0(self, x0, y0):
        F, p = self.F, self.p
        if self.literal:
            for y in range(y0, y0 + p):
                for x in range(x0, x0 + p):
                    if not F.visited(x, y):
                        continue
                    self.set_dir(0)
                    self.best_candidate(x, y)
            return
        # the same pixels in the same order; n is constant inside a level-0 window, so every pixel sees the same directions
        x1, y1 = min(x0 + p, F.W), min(y0 + p, F.H)
        if x1 <= x0 or y1 <= y0:
            return
        sub_any = F.any[y0:y1, x0:x1] & F.valid[y0:y1, x0:x1]
        ys, xs = np.nonzero(sub_any)
        if len(ys) == 0:
            return
        ys, xs = ys + y0, xs + x0
        self.set_dir(0)
        A = np.stack([F.A[l][ys, xs] for l in range(LEVELS)])
        G2 = np.stack([F.G2[l][ys, xs] for l in range(LEVELS)])
        PR = np.stack([projection(self.dir[l][0], self.dir[l][1], F.DX[l][ys, xs], F.DY[l][ys, xs]) for l in range(LEVELS)])
        pos = 0
        m = len(ys)
        while pos < m:
            # the first pixel at or after pos that some level accepts, and its lowest such level (levels with A false cannot
            # accept; a failed border makes A false for that level and every level above it)
            live = np.array([self.cand[l] != BLOCKED for l in range(LEVELS)])[:, None]
            w = np.array(self.weight)[:, None]
            acc = A[:, pos:] & live & (PR[:, pos:] > w)
            hit = acc.any(axis=0)
            if not hit.any():
                return
            j = int(np.argmax(hit))
            l = int(np.argmax(acc[:, j]))
            i = pos + j
            self.weight[l] = float(G2[l, i])
            self.cand[l] = int(ys[i]) * F.W + int(xs[i])
            for k in range(l + 1, LEVELS):
                self.cand[k] = BLOCKED
            pos = i + 1

    def window(self, level, x0, y0):
        F, p = self.F, self.p
        w = (1 << level) * p
        if not self.literal and not F.region_has_any(x0, y0, w):
            return   # no pixel inside can change any state: no emission, and the next window of this level resets its own
        self.cand[level] = NONE
        self.weight[level] = 0.0
        if level == 0:
            self.level0(x0, y0)
        else:
            step = w // 2
            for y in (y0, y0 + step):
                for x in (x0, x0 + step):
                    if not F.visited(x, y):
                        continue
                    self.set_dir(level)
                    self.window(level - 1, x, y)
        c = self.cand[level]
        if c >= 0 and c % F.W > 0:
            self.features.append((c, level))
            if level + 1 < LEVELS:
                self.weight[level + 1] = 1e10

    def top(self, x0, y0):
        self.window(LEVELS - 1, x0, y0)


def top_windows(W, H, p):
    step = (1 << (LEVELS - 1)) * p
    return [(x, y) for y in range(0, H, step) for x in range(0, W, step)]


def walk(F, p, pattern, literal=False):
    """one pass of findFeatures: [(pixel index, level)] in emission order"""
    wk = _Walker(F, p, pattern, literal)
    for x, y in top_windows(F.W, F.H, p):
        wk.top(x, y)
    return wk.features


def walk_literal(F, p, pattern):
    return walk(F, p, pattern, literal=True)


def walk_top(F, p, pattern, x0, y0, n0):
    """one top window alone, started with n0 features already emitted: [(pixel index, level)]"""
    wk = _Walker(F, p, pattern)
    wk.features = [None] * n0
    wk.top(x0, y0)
    return wk.features[n0:]


def walk_sub(F, p, pattern, x0, y0, k, n0):
    """level-2 window k = 4 c3 + c2 of the top window at (x0, y0) alone, started with n0 features emitted; levels 3 and 4 start
    fresh and emit nothing (their records decide only their own emissions)"""
    wk = _Walker(F, p, pattern)
    wk.features = [None] * n0
    c3, c2 = k >> 2, k & 3
    x3, y3 = x0 + (c3 & 1) * 8 * p, y0 + (c3 >> 1) * 8 * p
    x2, y2 = x3 + (c2 & 1) * 4 * p, y3 + (c2 >> 1) * 4 * p
    if F.visited(x3, y3) and F.visited(x2, y2):
        wk.window(2, x2, y2)
    return wk.features[n0:]


def ideal_potential(ratio, p):
    return max(1, int(math.sqrt(1.0 / ratio) * (p + 1) - 1))


def point_ratio(desired, found):
    return desired / float(found) if found > 0 else math.inf


class EigenExtractorModel:
    """EigenTrackingFeaturesExtractor: the potential persists across extract() calls.  `walker(F, p, pattern)` runs one pass."""

    def __init__(self, width, height, density, walker=walk):
        self.W, self.H, self.density = int(width), int(height), float(density)
        self.walker = walker
        self.initialized, self.potential, self.found_last = False, INITIAL_POTENTIAL, 0
        self.pattern = random_pattern(self.W * self.H)
        self.last_features = []
        self.stats = dict(passes=0, potentials=[0, 0], found=[0, 0])

    def state(self):
        return dict(initialized=self.initialized, grad_norm_threshold=0, window_size=self.potential, point_density=self.density,
                    found_last=self.found_last)

    def fields(self, img, mask=None):
        from oracle import pyoracle as po
        infos, _ = po.build_pyramid(img, levels=LEVELS)
        valid = fm.eroded_valid(mask, (self.H, self.W))
        tmap = threshold_map(infos[0][..., 1], infos[0][..., 2], valid)
        return Fields(infos, tmap, valid)

    def extract_fields(self, F):
        """-> (n, 2) float64 (x, y)"""
        stats = dict(passes=0, potentials=[0, 0], found=[0, 0])
        for k in range(2):
            feats = self.walker(F, self.potential, self.pattern)
            found = len(feats)
            stats["passes"] += 1
            stats["potentials"][k] = self.potential
            stats["found"][k] = found
            ratio = point_ratio(self.density, found)
            ideal = ideal_potential(ratio, self.potential)
            if k == 0 and ratio > 1.25 and self.potential > 1:
                self.potential = min(ideal, self.potential - 1)
            elif k == 0 and ratio < 0.25:
                self.potential = max(ideal, self.potential + 1)
            else:
                break
        self.initialized = True
        self.found_last = found
        self.stats = stats
        if ratio < 0.95:
            feats = [f for f in feats if int(self.pattern[f[0]]) <= int(255.0 * ratio)]
        self.last_features = feats
        idx = np.array([f[0] for f in feats], dtype=np.int64)
        return np.stack([idx % self.W, idx // self.W], axis=1).astype(np.float64).reshape(-1, 2)

    def extract(self, img, mask=None):
        return self.extract_fields(self.fields(img, mask))


# ---- the order-free formulation the device runs (features_eigen.hip) ----

def pixel_bits(F):
    """per pixel and level: possible_l = visited-by-own-mask and A_l; certain_l = possible_l and no direction of the 16 gives an
    exactly zero projection (so the projection is > 0 whatever pattern byte picks the direction)"""
    poss, cert = [], []
    for l in range(LEVELS):
        p = F.A[l] & F.valid
        nz = np.ones_like(p)
        for c, s in DIRECTIONS:
            nz &= projection(c, s, F.DX[l], F.DY[l]) != 0
        poss.append(p)
        cert.append(p & nz)
    return poss, cert


class ParallelPrototype:
    """Per top window T, the number of emissions E(T) without knowing n:
      inside a level-L window W, "something below L was accepted" holds exactly when some visited pixel P and level l < L have
      A_l(P) and a non-zero projection (the first such pair in traversal order is accepted: nothing can block it), and W emits
      exactly when that is false and some visited P has A_L(P) with a non-zero projection.  The projection is zero only for
      directions in a pixel's zero set, so each of these existence facts is certain (some pixel with an empty zero set), impossible
      (no pixel with A) or undetermined.  T is determined when every emission decision inside it is.
    Determined windows get their start count from an exclusive scan; undetermined ones are walked in order once their start is
    known (`chained`); then every T walks from its start independently.  A level's record decides only that level's emission and
    blocks nothing below it, so a determined T in which no level-3 or level-4 window may emit is walked as its 16 level-2 windows,
    each from the start count its predecessors' counts give."""

    def __init__(self, F, p, pattern):
        self.F, self.p, self.pattern = F, p, pattern
        self.poss, self.cert = pixel_bits(F)

    def _window_bits(self, x0, y0):
        """OR of (possible, certain) per level over the visited pixels of the level-0 window at (x0, y0)"""
        F, p = self.F, self.p
        x1, y1 = min(x0 + p, F.W), min(y0 + p, F.H)
        if x1 <= x0 or y1 <= y0:
            return np.zeros(LEVELS, bool), np.zeros(LEVELS, bool)
        return (np.array([self.poss[l][y0:y1, x0:x1].any() for l in range(LEVELS)]),
                np.array([self.cert[l][y0:y1, x0:x1].any() for l in range(LEVELS)]))

    def count(self, x0, y0, level=LEVELS - 1):
        """-> (possible[5], certain[5], E, undetermined, high) of the window (its corner is visited); high = some window of level 3
        or 4 in it may emit"""
        if level == 0:
            poss, cert = self._window_bits(x0, y0)
            E, und, high = 0, False, False
        else:
            poss, cert = np.zeros(LEVELS, bool), np.zeros(LEVELS, bool)
            E, und, high = 0, False, False
            step = (1 << level) * self.p // 2
            for y in (y0, y0 + step):
                for x in (x0, x0 + step):
                    if not self.F.visited(x, y):
                        continue
                    cp, cc, ce, cu, ch = self.count(x, y, level - 1)
                    poss |= cp
                    cert |= cc
                    E += ce
                    und |= cu
                    high |= ch
        low_poss, low_cert = poss[:level].any(), cert[:level].any()
        emit_cert = (not low_poss) and cert[level]
        emit_poss = (not low_cert) and poss[level]
        return poss, cert, E + int(emit_cert), und or (emit_poss and not emit_cert), high or (level >= 3 and emit_poss)

    def level2_counts(self, x0, y0):
        """the emissions of the 16 level-2 windows of a top window, in walk order (0 for one not visited)"""
        out = []
        for k in range(16):
            c3, c2 = k >> 2, k & 3
            x3, y3 = x0 + (c3 & 1) * 8 * self.p, y0 + (c3 >> 1) * 8 * self.p
            x2, y2 = x3 + (c2 & 1) * 4 * self.p, y3 + (c2 >> 1) * 4 * self.p
            visited = self.F.visited(x3, y3) and self.F.visited(x2, y2)
            out.append(self.count(x2, y2, 2)[2] if visited else 0)
        return out

    def run(self):
        """-> (features [(pixel index, level)], chained windows, per-T (E, determined))"""
        tops = top_windows(self.F.W, self.F.H, self.p)
        counts = [self.count(x, y) for x, y in tops]
        start, n, chained = [], 0, 0
        for (x, y), (_, _, E, und, _) in zip(tops, counts):
            start.append(n)
            if und:
                chained += 1
                n += len(walk_top(self.F, self.p, self.pattern, x, y, n))
            else:
                n += E
        out = [None] * n
        self.split = 0
        for (x, y), s, c in zip(tops, start, counts):
            if not c[3] and not c[4]:
                self.split += 1
                for k, e2 in enumerate(self.level2_counts(x, y)):
                    f = walk_sub(self.F, self.p, self.pattern, x, y, k, s)
                    assert len(f) == e2, (x, y, k, len(f), e2)
                    out[s:s + e2] = f
                    s += e2
            else:
                f = walk_top(self.F, self.p, self.pattern, x, y, s)
                out[s:s + len(f)] = f
        return out, chained, [(c[2], not c[3]) for c in counts]
