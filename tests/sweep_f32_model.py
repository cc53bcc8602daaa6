"""One sweep of the bundle-adjustment window in plain numpy, every quantity with a running bound on what the device's fp32 evaluation may
differ from it (no GPU, nothing taken from the device but the state and the texels a caller passes in).

The central values follow the expression trees of sweepKernel / fejKernel in dsopp_amd/csrc/pba_kernels.hpp: the pair constants M, U, tl,
fxt.., s, b_t, b_r, sigma_r, b_r0, Adj are computed here in float64 from poses, intrinsics, exposures and affine states (oracle/spec.py:
relative_pose, adjoint), the per-pixel chain is restated operation by operation.  Every quantity is an EV: (value in float64, bound >= 0
on |device - value|).  The bound is propagated mechanically:

  unit roundoff   u = 2^-24.
  conversions     u |x| for every conversion of a constant or operand to fp32 (S(Pm->M[0]), static_cast<S>(idepth_d + idepth_step_d), the
                  landmark's u, v, patch_k).  The pair constants are float64 results of the device's own pose arithmetic: they carry
                  SLACK * max|M| (resp. U) on top.
  + - *           the propagated bound of the exact result (a product carries |a| eb + |b| ea + ea eb) plus u (|result| + that bound).
                  A result that is exact - operands without bound and an exact result that fp32 represents, such as the integer
                  landmark coordinate plus the integer pattern offset - is charged nothing: fp32 arithmetic is exact there, and the
                  reference-side ROI decisions of landmarks ON a limit are decided.
  FMA             contraction only removes roundings: covered.
  divisions       dsopp_amd/csrc/build.sh compiles pba.hip with -O3 and neither -ffast-math nor -fno-hip-fp32-correctly-rounded-divide-sqrt.
                  hipcc's default for HIP is -fhip-fp32-correctly-rounded-divide-sqrt, fp32 denormals are on for gfx9: `1.0f / x`
                  (fastRcp(float)) and `/ Z` (non-FEJ and WFEJ paths) are the IEEE division expansion (v_div_scale / v_div_fmas /
                  v_div_fixup), correctly rounded: u |result| like any other operation.  (A two-line kernel compiled with these flags
                  shows it: both quotients end in v_div_fixup_f32, .amdhsa_float_denorm_mode_32 is 3.)
  bilinear        |B(p') - B(p)| <= Lx |du| + Ly |dv| with Lx (Ly) the largest absolute difference of horizontally (vertically) adjacent
                  texels over the 3 x 3 cells around the sample - the interpolant is continuous across cell borders, so the device may
                  sit in a neighbouring cell.  On top the device's own roundings at ITS position (dx = tu - ix is exact): the weights
                  carry 1 (w11 = dxdy), 2, 2 (dy - dxdy, dx - dxdy) and 4 (w00 = 1 - dx - dy + dxdy) roundings of quantities <= 1, each
                  product one more, the 3 additions one each of partial sums <= max|texel|: (9 + 4 + 3) u max|texel| = 16 u max|texel|
                  over the 4 x 4 texels, times (1 + 1e-3).
  fp64 parts      sum8, Huber, gj, the Gram contraction, assembly and Schur complement carry the fp32 bounds linearly (products as
                  above), through Huber by its Lipschitz constants (|dE/dr2| <= 1/2, |dw/dr2| <= sigma / (2 max(r2, sigma^2)^1.5)) and
                  through 1 / H_dd by e / (H (H - e)).  Every fp64 sum adds SLACK = 1e-12 times the sum of |terms| for round-off and
                  accumulation order; the u^2 terms are carried exactly by the product rule.

Decisions carry their margin: |value - limit| of the reference-side ROI on pu, pv; validIdepth; z > 0; the target-side ROI limits 4 and
W - 5 / H - 5; the mask lookup (distance of the fractional position from .5, where the candidate texels' mask values differ); for the
first-estimate-Jacobians item test the same on tuf, tvf and u +- 2, v +- 2.  An item is DECIDED when every margin of every one of its 8
pixels exceeds that pixel's bound (a value without bound is decided whatever its margin: it is the device's value).  An UNDECIDED item
contributes both outcomes: every sum it enters keeps the central outcome and widens by |contribution| + bound.

The residual statuses a sweep starts from are part of the model as well (push_statuses): pushing a window's third keyframe evaluates and
accepts the pairs of the first two, in the window's arithmetic.

compare() is the one comparison of device outputs with model outputs: tests/test_gpu_sweep_f32.py feeds it the HIP window's outputs,
tests/test_sweep_f32_model.py the model's own central values computed with a deliberate mistake (DEFECTS).
"""
import dataclasses

import numpy as np

from oracle import spec

U32 = 2.0 ** -24
U64 = 2.0 ** -53
SLACK = 1e-12
OX = np.array([0, -1, 1, -2, 0, 2, -1, 0], dtype=np.float64)     # pattern.hpp:21-32 (kPatX, kPatY)
OY = np.array([2, 1, 1, 0, 0, 0, -1, -2], dtype=np.float64)
STATUS_OK, STATUS_OOB = 0, 3
DEFECTS = ("mask_truncated", "weights_swapped", "plane_tile_4x2", "roi_upper_w4", "no_b_t", "g2_sign")
_INF = np.inf


def _clean(e):
    """0 * inf = nan in a bound means 'no bound'"""
    return np.where(np.isnan(e), _INF, e)


class EV:
    """value and bound on the device's deviation from it; + - * are EXACT arithmetic (fp64 parts), F32 adds the roundings"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.asarray(e, dtype=np.float64)

    @staticmethod
    def of(x):
        return x if isinstance(x, EV) else EV(x)

    def __add__(self, o):
        o = EV.of(o)
        return EV(self.v + o.v, self.e + o.e)

    __radd__ = __add__

    def __sub__(self, o):
        o = EV.of(o)
        return EV(self.v - o.v, self.e + o.e)

    def __neg__(self):
        return EV(-self.v, self.e)

    def __mul__(self, o):
        o = EV.of(o)
        with np.errstate(invalid="ignore"):
            return EV(self.v * o.v, _clean(np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e))

    __rmul__ = __mul__

    def __getitem__(self, k):
        return EV(self.v[k], np.broadcast_to(self.e, self.v.shape)[k])

    def sum(self, axis=None):
        """an fp64 sum: the bounds add, plus SLACK * sum |terms| for round-off and order"""
        e = np.broadcast_to(self.e, self.v.shape)
        return EV(self.v.sum(axis), e.sum(axis) + SLACK * np.abs(self.v).sum(axis))


def stack(evs, axis=-1):
    shape = np.broadcast_shapes(*[x.v.shape for x in evs])
    return EV(np.stack([np.broadcast_to(x.v, shape) for x in evs], axis), np.stack([np.broadcast_to(x.e, shape) for x in evs], axis))


def matmul_exact(A, B, left=True):
    """A @ B (left) or B @ A with A exact fp64 constants and B an EV"""
    a = np.abs(A)
    if left:
        return EV(A @ B.v, a @ np.broadcast_to(B.e, B.v.shape) + SLACK * (a @ np.abs(B.v)))
    return EV(B.v @ A, np.broadcast_to(B.e, B.v.shape) @ a + SLACK * (np.abs(B.v) @ a))


class F32:
    """the roundings of the device's S = float arithmetic (u = U32), or of S = double (u = U64: the model against the fp64 oracle)"""

    def __init__(self, u=U32):
        self.u = u
        self.exact_aware = u == U32

    def rnd(self, x):
        with np.errstate(invalid="ignore", over="ignore"):
            charge = self.u * (np.abs(x.v) + x.e)
            # (what fp32 represents, fp64 represents: the same test serves u = U64)
            exact = (x.e == 0) & (x.v.astype(np.float32).astype(np.float64) == x.v)
            charge = np.where(exact, 0.0, charge)
            return EV(x.v, _clean(x.e + charge))

    def conv(self, x, extra=0.0):
        return self.rnd(EV(x, extra))

    def add(self, a, b):
        return self.rnd(EV.of(a) + b)

    def sub(self, a, b):
        return self.rnd(EV.of(a) - b)

    def mul(self, a, b):
        return self.rnd(EV.of(a) * b)

    def div(self, a, b):
        """a / b, correctly rounded (see the module docstring): |a'/b' - a/b| <= (ea + |a/b| eb) / (|b| - eb)"""
        a, b = EV.of(a), EV.of(b)
        with np.errstate(divide="ignore", invalid="ignore"):
            v = a.v / b.v
            den = np.abs(b.v) - b.e
            e = np.where(den > 0, (a.e + np.abs(v) * b.e) / den, _INF)
        return self.rnd(EV(v, _clean(e)))

    def affine3(self, c0, c1, c2, c3, pu, pv, idp):
        """c0 * pu + c1 * pv + (c2 + c3 * idepth) in the kernel's association"""
        return self.add(self.add(self.mul(c0, pu), self.mul(c1, pv)), self.add(c2, self.mul(c3, idp)))


@dataclasses.dataclass
class ModelFrame:
    T0: np.ndarray              # 4 x 4 pose at the linearisation point
    intr: np.ndarray            # fx, fy, cx, cy
    exposure: float
    ab0: np.ndarray
    fixed: bool
    texels: np.ndarray          # H x W x 3 float64 holding the values the device holds (float32-representable for the f32 model)
    mask: np.ndarray            # H x W bool (True = valid) or None
    uv: np.ndarray
    patch: np.ndarray           # n x 8
    f32_plane: bool             # the residual-only sweep reads the 4 x 4-tiled 32-bit plane: lowest mantissa bit cleared

    @property
    def size(self):
        return self.texels.shape[1], self.texels.shape[0]


@dataclasses.dataclass
class ModelWindow:
    frames: list
    sigma_huber: float = 20.0
    affine_regularizer: tuple = (1e12, 1e8)
    fixed_regularizer: float = 1e16


@dataclasses.dataclass
class State:
    eps: np.ndarray             # F x 8
    step: np.ndarray            # F x 8
    idepth: list                # per frame
    idepth_step: list

    @staticmethod
    def initial(idepths):
        F = len(idepths)
        return State(np.zeros((F, 8)), np.zeros((F, 8)), [np.asarray(d, dtype=np.float64).copy() for d in idepths],
                     [np.zeros(len(d)) for d in idepths])


def model_window(scene, texels=None, f32=True):
    """ModelWindow of a tests/sweep_edge_scenes.py scene.  texels: one H x W x 3 array per keyframe (the F32 device pyramid's level for the
    level scenes); default frames[i].pixelinfo, rounded to float32 when f32 (what Pyramid.set_level stores)"""
    from dsopp_amd import synthetic as syn
    frames = []
    for i, f in enumerate(scene.window.frames):
        tex = np.asarray(f.pixelinfo if texels is None else texels[i], dtype=np.float64)
        if f32:
            tex = tex.astype(np.float32).astype(np.float64)
        mask = None if scene.masks is None else (np.asarray(scene.masks[i]) != 0)
        frames.append(ModelFrame(spec.quat_to_mat(syn.mat_to_params(f.T_w_c_init)), np.asarray(scene.intrinsics, dtype=np.float64),
                                 float(f.exposure), np.asarray(f.affine_init, dtype=np.float64), bool(f.fixed), tex, mask,
                                 np.asarray(f.uv, dtype=np.float64), np.asarray(f.patch, dtype=np.float64), f32))
    return ModelWindow(frames)


def initial_state(scene):
    return State.initial([f.idepth_init for f in scene.window.frames])


# ---------------------------------------------------------------------------------------------------------------------------------------
# pair constants (computePairConst, buildProjectionMatrices) in float64
# ---------------------------------------------------------------------------------------------------------------------------------------
def _projection(T, ir, it):
    """U = [R|t] Kinv_r, M = K_t U (camera_reproject.hpp:235-260), row-major 3 x 4"""
    fxr, fyr, cxr, cyr = ir
    fxt, fyt, cxt, cyt = it
    U = np.zeros((3, 4))
    U[:, 0] = T[:3, 0] / fxr
    U[:, 1] = T[:3, 1] / fyr
    U[:, 2] = T[:3, 0] * (-cxr / fxr) + T[:3, 1] * (-cyr / fyr) + T[:3, 2]
    U[:, 3] = T[:3, 3]
    M = np.stack([fxt * U[0] + cxt * U[2], fyt * U[1] + cyt * U[2], U[2]])
    return U, M


def pair_constants(win, state, r, t, fej):
    fr, ft = win.frames[r], win.frames[t]
    xr, xt = state.eps[r] + state.step[r], state.eps[t] + state.step[t]
    T0 = np.linalg.inv(ft.T0) @ fr.T0
    T = spec.exp_se3(-xt[:6]) @ T0 @ spec.exp_se3(xr[:6])
    _, M = _projection(T, fr.intr, ft.intr)
    a_r, a_t = fr.ab0[0] + xr[6], ft.ab0[0] + xt[6]
    P = dict(M=M, s=(ft.exposure / fr.exposure) * np.exp(a_t - a_r), b_t=ft.ab0[1] + xt[7], b_r=fr.ab0[1] + xr[7], intr_t=ft.intr)
    Tlin = T0 if fej else T
    P["U"], _ = _projection(Tlin, fr.intr, ft.intr)
    P["U0"], _ = _projection(T0, fr.intr, ft.intr)     # the first-estimate item test always reprojects at the linearisation point
    P["Adj"] = spec.adjoint(Tlin)
    P["tl"] = Tlin[:3, 3]
    if fej:
        last = max(k for k in range(len(win.frames)) if k != r)     # full clique: every other frame is connected
        fl = win.frames[last]
        P["s0"] = (ft.exposure / fr.exposure) * np.exp(ft.ab0[0] - fr.ab0[0])
        P["b_r0"] = fr.ab0[1]
        P["sigma_r"] = (fl.exposure / fr.exposure) * np.exp(fl.ab0[0] - fr.ab0[0])
    else:
        P["s0"], P["b_r0"], P["sigma_r"] = P["s"], P["b_r"], P["s"]
    return P


# ---------------------------------------------------------------------------------------------------------------------------------------
# texels: the tiled intensity plane, Lipschitz and magnitude maps
# ---------------------------------------------------------------------------------------------------------------------------------------
def _clear_lowest_bit(x32):
    return (np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFFFFFE)).view(np.float32)


class _Image:
    """what a sweep reads of one frame: texel lanes (linearisation) or the tiled plane (residual-only), with the maps of the bound"""

    def __init__(self, frame, plane):
        tex = frame.texels
        self.H, self.W = tex.shape[:2]
        self.mask = np.ones((self.H, self.W), dtype=bool) if frame.mask is None else frame.mask
        self.has_mask = frame.mask is not None
        self.plane = plane
        if plane:
            inten = tex[..., 0]
            if frame.f32_plane:      # buildIntensityPlaneKernel(const Texel<float>*, ...): bits & ~1u, mask into bit 0
                inten = _clear_lowest_bit(inten).astype(np.float64)
            self.tiles_x, tiles_y = (self.W + 3) // 4, (self.H + 3) // 4
            n = self.tiles_x * tiles_y * 16
            self.pl_val, self.pl_mask = np.zeros(n), np.zeros(n, dtype=bool)
            ys, xs = np.mgrid[0:self.H, 0:self.W]
            idx = self.tile_index(xs, ys)
            self.pl_val[idx] = inten
            self.pl_mask[idx] = self.mask
            self.chan = [inten]
        else:
            self.chan = [tex[..., c] for c in range(3)]
        self.maps = [self._maps(c) for c in self.chan]

    def tile_index(self, x, y, shape_4x2=False):
        if shape_4x2:   # the f64 plane's tile shape (pba_kernels.hpp:704) applied to the f32 plane
            return np.minimum(((y >> 1) * self.tiles_x + (x >> 2)) * 8 + ((y & 1) << 2) + (x & 3), len(self.pl_val) - 1)
        return ((y >> 2) * self.tiles_x + (x >> 2)) * 16 + ((y & 3) << 2) + (x & 3)

    def _maps(self, c):
        """per cell (iy, ix): Lx, Ly over the 3 x 3 cells around it, max |texel| over their 4 x 4 texels"""
        H, W = c.shape

        def window_max(a, rows, cols):   # out[iy, ix] = max a[iy + rows, ix + cols] (zero outside the array; a >= 0)
            out = np.zeros((H, W))
            p = np.pad(a, ((3, 3), (3, 3)))
            for dy in rows:
                for dx in cols:
                    out = np.maximum(out, p[3 + dy:3 + dy + H, 3 + dx:3 + dx + W])
            return out
        dh = np.zeros((H, W))
        dh[:, :-1] = np.abs(np.diff(c, axis=1))      # dh[y, x] = |c[y, x + 1] - c[y, x]|
        dv = np.zeros((H, W))
        dv[:-1, :] = np.abs(np.diff(c, axis=0))
        return (window_max(dh, range(-1, 3), range(-1, 2)), window_max(dv, range(-1, 2), range(-1, 3)),
                window_max(np.abs(c), range(-1, 3), range(-1, 3)))

    def sample(self, A, tu, tv, channels, defect):
        """bilinear samples of `channels` at (tu, tv) (EVs), as the kernel blends them; (list of EV, ix, iy)"""
        with np.errstate(invalid="ignore"):
            fin = np.isfinite(tu.v) & np.isfinite(tv.v)
            tuv, tvv = np.where(fin, tu.v, 0.0), np.where(fin, tv.v, 0.0)
            ix = np.clip(np.floor(tuv), 0, self.W - 2).astype(np.int64)
            iy = np.clip(np.floor(tvv), 0, self.H - 2).astype(np.int64)
            dx, dy = np.clip(tuv - ix, 0, 1), np.clip(tvv - iy, 0, 1)
            dxdy = dx * dy
            w11, w01, w10, w00 = dxdy, dy - dxdy, dx - dxdy, 1 - dx - dy + dxdy
            if defect == "weights_swapped":
                w01, w10 = w10, w01
            pos_e = np.where(fin & (tu.e < 1) & (tv.e < 1), 1.0, _INF)
            out = []
            for c in channels:
                if self.plane:
                    at = lambda x, y: self.pl_val[self.tile_index(x, y, defect == "plane_tile_4x2")]   # noqa: E731
                else:
                    at = lambda x, y: self.chan[c][y, x]   # noqa: E731
                val = w11 * at(ix + 1, iy + 1) + w01 * at(ix, iy + 1) + w10 * at(ix + 1, iy) + w00 * at(ix, iy)
                Lx, Ly, amax = (m[iy, ix] for m in self.maps[c])
                e = (Lx * tu.e + Ly * tv.e) * pos_e + 16 * A.u * amax * (1 + 1e-3)
                out.append(EV(val, _clean(e)))
        return out, ix, iy

    def mask_lookup(self, A, tu, tv, ix, iy, defect):
        """(mask value at floor(t + 0.5), decided): the lookup is decided unless a candidate texel with another mask value is within the
        position's bound of the rounding limit"""
        if not self.has_mask and defect != "plane_tile_4x2":
            return np.ones(tu.v.shape, dtype=bool), np.ones(tu.v.shape, dtype=bool)
        with np.errstate(invalid="ignore"):
            hu, hv = A.add(tu, 0.5), A.add(tv, 0.5)             # floor(tu + S(0.5)): the sum is one more rounding
            fin = np.isfinite(hu.v) & np.isfinite(hv.v)
            huv, hvv = np.where(fin, hu.v, 0.0), np.where(fin, hv.v, 0.0)
            rx, ry = np.floor(huv).astype(np.int64), np.floor(hvv).astype(np.int64)
            if defect == "mask_truncated":
                rx, ry = ix.copy(), iy.copy()
            fx, fy = huv - np.floor(huv), hvv - np.floor(hvv)
            ax, ay = np.where(fx < 0.5, rx - 1, rx + 1), np.where(fy < 0.5, ry - 1, ry + 1)
            d_x, d_y = np.minimum(fx, 1 - fx), np.minimum(fy, 1 - fy)

            def m(x, y):
                x, y = np.clip(x, 0, self.W - 1), np.clip(y, 0, self.H - 1)
                if self.plane:
                    return self.pl_mask[self.tile_index(x, y, defect == "plane_tile_4x2")]
                return self.mask[y, x]
            m0 = m(rx, ry)
            margin = np.minimum(np.where(m(ax, ry) != m0, d_x, _INF),
                                np.minimum(np.where(m(rx, ay) != m0, d_y, _INF), np.where(m(ax, ay) != m0, np.maximum(d_x, d_y), _INF)))
            decided = fin & (margin > np.maximum(hu.e, hv.e))
        return m0, decided


# ---------------------------------------------------------------------------------------------------------------------------------------
# the sweep
# ---------------------------------------------------------------------------------------------------------------------------------------
class _Decisions:
    def __init__(self, shape):
        self.ok = np.ones(shape, dtype=bool)
        self.decided = np.ones(shape, dtype=bool)

    def _cmp(self, x, limit, op):
        with np.errstate(invalid="ignore"):
            self.ok = self.ok & op(x.v, limit)
            self.decided = self.decided & ((np.abs(x.v - limit) > x.e) | ((x.e == 0) & np.isfinite(x.v)))

    def gt(self, x, limit):
        self._cmp(x, limit, np.greater)

    def lt(self, x, limit):
        self._cmp(x, limit, np.less)

    def roi(self, u, v, W, H, defect=None):
        """insideROI (device_geom.hpp:8-11): inclusive limits 4 and W - 5 / H - 5"""
        up = 4 if defect == "roi_upper_w4" else 5
        self._cmp(u, 4.0, np.greater_equal)
        self._cmp(v, 4.0, np.greater_equal)
        self._cmp(u, float(W - up), np.less_equal)
        self._cmp(v, float(H - up), np.less_equal)

    def valid_idepth(self, A, d):
        """validIdepth (device_geom.hpp:13-16); the limits are S(-1e-4) and S(1010)"""
        lo, hi = (np.float64(np.float32(-1e-4)), np.float64(np.float32(1010.0))) if A.exact_aware else (-1e-4, 1010.0)
        self.gt(d, lo)
        self.lt(d, hi)


def _consts(A, arr):
    """the pair's float64 constants converted to S, each with the fp64 slack of the device's own pose arithmetic"""
    arr = np.asarray(arr, dtype=np.float64)
    return A.conv(arr, SLACK * np.abs(arr).max())


def _sweep_pair(A, win, P, r, t, state, fej_idepth, fej, linearize, defect, images, status, status_decided):
    fr, ft = win.frames[r], win.frames[t]
    n = len(fr.uv)
    Wr, Hr = fr.size
    Wt, Ht = ft.size
    u, v = A.conv(fr.uv[:, 0:1]), A.conv(fr.uv[:, 1:2])
    pu, pv = A.add(u, OX[None, :]), A.add(v, OY[None, :])
    idp = A.conv((state.idepth[r] + state.idepth_step[r])[:, None])
    fxt, fyt, cxt, cyt = (_consts(A, P["intr_t"])[k] for k in range(4))
    M, U = _consts(A, P["M"]), _consts(A, P["U"])
    dec = _Decisions((n, 8))
    dec.valid_idepth(A, idp)
    dec.roi(pu, pv, Wr, Hr, defect)
    if not linearize or fej:      # reproject without Jacobians: M and fastRcp(float) = 1.0f / z (pba_kernels.hpp:663-669)
        x, y, z = (A.affine3(M[i, 0], M[i, 1], M[i, 2], M[i, 3], pu, pv, idp) for i in range(3))
        iz = A.div(1.0, z)
        tu, tv = A.mul(x, iz), A.mul(y, iz)
        dec.gt(z, 0.0)
    else:                         # non-FEJ linearisation: positions from the Jacobian path, U and / Z (pba_kernels.hpp:672-677)
        X, Y, Z = (A.affine3(U[i, 0], U[i, 1], U[i, 2], U[i, 3], pu, pv, idp) for i in range(3))
        tu = A.div(A.add(A.mul(fxt, X), A.mul(cxt, Z)), Z)
        tv = A.div(A.add(A.mul(fyt, Y), A.mul(cyt, Z)), Z)
        dec.gt(Z, 0.0)
    dec.roi(tu, tv, Wt, Ht, defect)
    img = images(t, not linearize)
    samples, ix, iy = img.sample(A, tu, tv, [0, 1, 2] if linearize else [0], defect)
    mval, mdec = img.mask_lookup(A, tu, tv, ix, iy, defect)
    pos_ok = dec.ok                      # a lane only touches the image when its own pixel is inside the ROI
    dec.ok = pos_ok & mval
    dec.decided = dec.decided & np.where(pos_ok, mdec, True)
    item_ok, item_dec = dec.ok.all(axis=1), dec.decided.all(axis=1)
    fej_ok = np.ones(n, dtype=bool)
    if fej:   # firstEstimateJacobians_ (fejKernel / the WFEJ block, pba_kernels.hpp:273-287, 761-769) at the inverse-depth snapshot
        U0 = _consts(A, P["U0"])
        idf = A.conv(fej_idepth[r][:, None])
        X, Y, Z = (A.affine3(U0[i, 0], U0[i, 1], U0[i, 2], U0[i, 3], pu, pv, idf) for i in range(3))
        tuf = A.div(A.add(A.mul(fxt, X), A.mul(cxt, Z)), Z)
        tvf = A.div(A.add(A.mul(fyt, Y), A.mul(cyt, Z)), Z)
        df = _Decisions((n, 8))
        df.gt(Z, 0.0)
        df.roi(tuf, tvf, Wt, Ht, defect)
        df.valid_idepth(A, idf)
        df.roi(A.sub(u, 2.0), A.sub(v, 2.0), Wr, Hr, defect)
        df.roi(A.add(u, 2.0), A.add(v, 2.0), Wr, Hr, defect)
        fej_ok = df.ok.all(axis=1)
        item_ok, item_dec = item_ok & fej_ok, item_dec & df.decided.all(axis=1)
    # residual and Huber (pba_kernels.hpp:785-796), computed for every item: an undecided item needs its "inside" outcome
    b_t, s, b_r = _consts(A, P["b_t"]), _consts(A, P["s"]), _consts(A, P["b_r"])
    patch = A.conv(fr.patch)
    left = samples[0] if defect == "no_b_t" else A.sub(samples[0], b_t)
    res = A.sub(left, A.mul(s, A.sub(patch, b_r)))
    r2 = A.mul(res, res).sum(axis=1)
    sig = win.sigma_huber
    with np.errstate(invalid="ignore", divide="ignore"):
        hub = r2.v > sig * sig
        nrm = np.sqrt(np.maximum(r2.v, 0))
        energy = EV(np.where(hub, sig * nrm - 0.5 * sig * sig, 0.5 * r2.v), 0.5 * r2.e)
        energy = EV(energy.v, _clean(energy.e + SLACK * np.abs(energy.v)))
        wgt = EV(np.where(hub, sig / nrm, 1.0), r2.e * sig / (2 * np.maximum(np.maximum(r2.v - r2.e, 0), sig * sig) ** 1.5))
        wgt = EV(wgt.v, _clean(wgt.e + SLACK))
    # evaluate_jacobians.hpp:111-123: a failed item's candidate is OOB, a successful one is evaluated (candidate OK) if its status is OK
    # and keeps its candidate - the status it was accepted with - otherwise
    evaluate = item_ok & (status == STATUS_OK)
    item_dec = item_dec & status_decided
    out = dict(ok=item_ok, evaluate=evaluate, decided=item_dec, fej_ok=fej_ok, energy=energy, weight=wgt.v, status=status,
               candidate=np.where(evaluate, STATUS_OK, np.where(item_ok, status, STATUS_OOB)).astype(np.uint8))
    if not linearize:
        return out
    # geometric Jacobians at the linearisation point (pba_kernels.hpp:809-831)
    idj = A.conv(fej_idepth[r][:, None]) if fej else idp
    X, Y, Z = (A.affine3(U[i, 0], U[i, 1], U[i, 2], U[i, 3], pu, pv, idj) for i in range(3))
    tl = _consts(A, P["tl"])
    rho = A.div(1.0, Z)
    b0, b1 = A.mul(X, rho), A.mul(Y, rho)
    du_id = A.mul(fxt, A.sub(A.mul(tl[0], rho), A.mul(tl[2], A.mul(rho, b0))))
    dv_id = A.mul(fyt, A.sub(A.mul(tl[1], rho), A.mul(tl[2], A.mul(rho, b1))))
    nid = A.mul(idj, rho)
    Iu, Iv = samples[1], samples[2]
    b0b1 = A.mul(b0, b1)
    g2b = A.mul(Iu, A.mul(fxt, A.mul(-nid, b0)))
    g = [A.mul(Iu, A.mul(fxt, nid)),
         A.mul(Iv, A.mul(fyt, nid)),
         A.add(A.mul(Iv, A.mul(fyt, A.mul(-nid, b1))), -g2b if defect == "g2_sign" else g2b),
         A.add(A.mul(Iv, A.mul(fyt, -A.add(A.mul(b1, b1), 1.0))), A.mul(Iu, A.mul(fxt, -b0b1))),
         A.add(A.mul(Iv, A.mul(fyt, b0b1)), A.mul(Iu, A.mul(fxt, A.add(A.mul(b0, b0), 1.0)))),
         A.add(A.mul(Iv, A.mul(fyt, b0)), A.mul(Iu, A.mul(fxt, -b1))),
         A.mul(_consts(A, P["sigma_r"]), A.sub(patch, _consts(A, P["b_r0"]))),
         EV(np.ones((n, 8)))]
    g = stack(g, axis=-1)                                     # n x 8 pixels x 8
    jdd = A.add(A.mul(Iu, du_id), A.mul(Iv, dv_id))           # evaluate_jacobians.hpp:165-174
    # fp64 from here.  An item enters with the factor `incl`: 1 / 0 where decided, the central outcome +- 1 where not
    incl = EV(evaluate.astype(np.float64), (~item_dec).astype(np.float64))
    w = EV(wgt.v, wgt.e) * incl                               # n
    wg = g * w[:, None, None]
    out["u"] = (wg * jdd[:, :, None]).sum(axis=1)             # n x 8: h_p block of the target is -u
    out["hdd"] = (jdd * jdd).sum(axis=1) * w
    out["bd"] = (jdd * res).sum(axis=1) * w
    out["G"] = (wg[:, :, :, None] * g[:, :, None, :]).sum(axis=(0, 1))      # 8 x 8
    out["q"] = (wg * res[:, :, None]).sum(axis=(0, 1))
    return out


@dataclasses.dataclass
class SweepResult:
    pairs: dict                  # (r, t) -> dict(ok, evaluate, decided, fej_ok, status, candidate, energy EV, weight[, u, hdd, bd, G, q])
    energy: EV                   # total, priors included
    count: tuple                 # (lowest, highest) number of valid residuals
    undecided: int
    items: int
    landmarks: dict = None       # r -> dict(hpib EV n x K, b_d EV, inv_hdd EV)
    system: tuple = None         # H_pp, b_pp, H_schur, b_schur as EVs


def sweep(win, state, fej, linearize=False, u=U32, defect=None, fej_idepth=None, statuses=None):
    """the residual-only sweep (calculate_energy) or the linearisation sweep with its reduction and assembly (linearize) of `win` at `state`.
    fej_idepth: the inverse depths of the first-estimate snapshot (begin()); default the state's own.
    statuses: {(r, t): (status per item, decided per item)} the sweep starts from (push_statuses); default all OK."""
    assert defect is None or defect in DEFECTS
    A = F32(u)
    F = len(win.frames)
    K = 8 * F
    fej_idepth = state.idepth if fej_idepth is None else fej_idepth
    cache = {}

    def images(t, plane):
        if (t, plane) not in cache:
            cache[(t, plane)] = _Image(win.frames[t], plane)
        return cache[(t, plane)]
    pairs, consts = {}, {}
    for r in range(F):
        for t in range(F):
            if r != t:
                consts[(r, t)] = pair_constants(win, state, r, t, fej)
                n = len(win.frames[r].uv)
                status, sdec = (np.zeros(n, dtype=np.uint8), np.ones(n, dtype=bool)) if statuses is None else statuses[(r, t)]
                pairs[(r, t)] = _sweep_pair(A, win, consts[(r, t)], r, t, state, fej_idepth, fej, linearize, defect, images, status, sdec)
    # totals (energyReduceKernel + priorEnergy; calculateLandmarksEnergy - problem.hpp:93-144)
    total, lo, hi, undecided, items = EV(0.0), 0, 0, 0, 0
    for p in pairs.values():
        incl = EV(p["evaluate"].astype(np.float64), (~p["decided"]).astype(np.float64))
        total = total + (p["energy"] * incl).sum()
        sure = p["decided"] & p["evaluate"] & (p["energy"].v > p["energy"].e)
        maybe = (~p["decided"]) | (p["evaluate"] & ~(p["energy"].v > p["energy"].e) & (p["energy"].v + p["energy"].e > 0))
        lo, hi = lo + int(sure.sum()), hi + int(sure.sum()) + int((maybe & ~sure).sum())
        undecided += int((~p["decided"]).sum())
        items += len(p["ok"])
    prior = 0.0
    for i, f in enumerate(win.frames):   # AffineBrightnessPrior::energyTerm - state_priors.hpp:87-90, at eps + step
        ab = f.ab0 + state.eps[i, 6:] + state.step[i, 6:]
        prior += 0.5 * float((ab * np.asarray(win.affine_regularizer) * ab).sum())
    total = EV(total.v + prior, total.e + SLACK * (abs(prior) + abs(total.v)))
    result = SweepResult(pairs, total, (lo, hi), undecided, items)
    if not linearize:
        return result
    # pose-pose system: H_tt = G, H_rr = T^T G T, H_rt = -T^T G, b_t = -q, b_r = T^T q with T = blockdiag(Adj, 1, s0)
    Hv, He, bv, be = np.zeros((K, K)), np.zeros((K, K)), np.zeros(K), np.zeros(K)

    def acc(rows, cols, x, sign=1.0):
        Hv[rows, cols] += sign * x.v
        He[rows, cols] += np.broadcast_to(x.e, x.v.shape)
    Ts = {}
    for (r, t), p in pairs.items():
        T = np.zeros((8, 8))
        T[:6, :6] = consts[(r, t)]["Adj"]
        T[6, 6], T[7, 7] = 1.0, consts[(r, t)]["s0"]
        Ts[(r, t)] = T
        rs, ts = slice(8 * r, 8 * r + 8), slice(8 * t, 8 * t + 8)
        G, q = p["G"], p["q"]
        TtG = matmul_exact(T.T, G)
        acc(ts, ts, G)
        acc(rs, rs, matmul_exact(T, TtG, left=False))
        acc(rs, ts, TtG, -1.0)
        acc(ts, rs, EV(TtG.v.T, TtG.e.T), -1.0)
        bv[ts] -= q.v
        be[ts] += q.e
        Tq = matmul_exact(T.T, q)
        bv[rs] += Tq.v
        be[rs] += Tq.e
    He += SLACK * np.abs(Hv)
    be = be + SLACK * np.abs(bv)
    for i, f in enumerate(win.frames):   # evaluateLinearSystemPrior - problem.hpp:37-77, added exactly
        d = np.arange(8 * i, 8 * i + 8)
        if f.fixed:
            Hv[d, d] += win.fixed_regularizer
            bv[d] += win.fixed_regularizer * state.eps[i]
        else:
            for a in range(2):
                Hv[d[6 + a], d[6 + a]] += win.affine_regularizer[a]
                bv[d[6 + a]] += win.affine_regularizer[a] * (f.ab0[a] + state.eps[i, 6 + a])
    He += SLACK * np.abs(Hv)
    be = be + SLACK * np.abs(bv)
    # per landmark: hpib, b_d, 1 / H_dd, and the Schur complement (hessian_block_evaluation.hpp:169-236)
    landmarks = {}
    Sv, Se, sbv, sbe = np.zeros((K, K)), np.zeros((K, K)), np.zeros(K), np.zeros(K)
    for r in range(F):
        n = len(win.frames[r].uv)
        hv, he = np.zeros((n, K)), np.zeros((n, K))
        hdd, bd = EV(np.zeros(n)), EV(np.zeros(n))
        for t in range(F):
            if t == r:
                continue
            p = pairs[(r, t)]
            ur = matmul_exact(Ts[(r, t)], p["u"], left=False)      # T^T u as a row: u @ T
            hv[:, 8 * t:8 * t + 8] -= p["u"].v
            he[:, 8 * t:8 * t + 8] += p["u"].e
            hv[:, 8 * r:8 * r + 8] += ur.v
            he[:, 8 * r:8 * r + 8] += ur.e
            hdd, bd = hdd + p["hdd"], bd + p["bd"]
        hpib = EV(hv, he + SLACK * np.abs(hv))
        hdd = EV(hdd.v, hdd.e + SLACK * np.abs(hdd.v))
        bd = EV(bd.v, bd.e + SLACK * np.abs(bd.v))
        with np.errstate(divide="ignore", invalid="ignore"):
            well = hdd.v > 1e-15                                   # kIdepthNullSpaceThreshold
            safe = hdd.v - hdd.e > 1e-15
            inv_v = np.where(well, 1.0 / hdd.v, 0.0)
            inv_e = np.where(well, np.where(safe, hdd.e / (hdd.v * (hdd.v - hdd.e)), _INF), np.where(hdd.e > 0, _INF, 0.0))
        inv = EV(inv_v, _clean(inv_e + SLACK * inv_v))
        landmarks[r] = dict(hpib=hpib, b_d=bd, inv_hdd=inv)
        ih = hpib * inv[:, None]
        S = (ih[:, :, None] * hpib[:, None, :]).sum(axis=0)
        sb = (ih * bd[:, None]).sum(axis=0)
        Sv, Se, sbv, sbe = Sv + S.v, Se + S.e, sbv + sb.v, sbe + sb.e
    result.landmarks = landmarks
    result.system = (EV(Hv, He), EV(bv, be), EV(Sv, _clean(Se + SLACK * np.abs(Sv))), EV(sbv, _clean(sbe + SLACK * np.abs(sbv))))
    return result


def push_statuses(win, state, fej, u=U32, defect=None):
    """the residual statuses a three-keyframe window starts a solve with.  Pushing the third keyframe evaluates the pairs of the first two
    (firstEstimateJacobians, then the linearisation sweep of the window's mode) and accepts their candidates
    (eigen_photometric_bundle_adjustment.cpp:119-141, foldMarginalized in pba.hip); the pairs with the third keyframe start OK.
    Returns {(r, t): (status, decided)}."""
    assert len(win.frames) == 3
    two = ModelWindow(win.frames[:2], win.sigma_huber, win.affine_regularizer, win.fixed_regularizer)
    st = State(state.eps[:2], state.step[:2], state.idepth[:2], state.idepth_step[:2])
    first = sweep(two, st, fej, linearize=True, u=u, defect=defect)
    out = {}
    for r in range(3):
        for t in range(3):
            if r != t:
                n = len(win.frames[r].uv)
                p = first.pairs.get((r, t))
                out[(r, t)] = (np.zeros(n, dtype=np.uint8), np.ones(n, dtype=bool)) if p is None else (p["candidate"], p["decided"])
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------------------------------------------------------------------
def as_device(energy_result, lin_result=None):
    """central values of the model in the shape of the device outputs compare() takes"""
    dev = dict(residuals={k: dict(candidate=p["candidate"].copy(), status=p["status"].copy(),
                                  energy=np.where(p["evaluate"], p["energy"].v, 0.0)) for k, p in energy_result.pairs.items()},
               energy=float(energy_result.energy.v),
               count=int(sum((p["evaluate"] & (p["energy"].v > 0)).sum() for p in energy_result.pairs.values())))
    if lin_result is not None:
        dev["system"] = tuple(x.v.copy() for x in lin_result.system)
        dev["landmarks"] = {r: {k: x.v.copy() for k, x in lm.items()} for r, lm in lin_result.landmarks.items()}
    return dev


def _ratio(diff, bound):
    """largest |difference| / bound (0 / 0 = 0, x / 0 = inf, anything / inf = 0)"""
    diff, bound = np.abs(np.asarray(diff, dtype=np.float64)), np.broadcast_to(np.asarray(bound, dtype=np.float64), np.shape(diff))
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(diff == 0, 0.0, np.where(np.isinf(bound), 0.0, diff / bound))
    return float(np.max(q)) if q.size else 0.0


def compare(dev, energy_result, lin_result=None):
    """device outputs against model outputs.  dev: dict(residuals={(r, t): dict(status, candidate, energy)}, energy, count[, system=(H_pp,
    b_pp, H_schur, b_schur), landmarks={r: dict(hpib, b_d, inv_hdd)}]).  Returns (failures: list of str, ratios: {quantity: largest
    |difference| / bound}); the check passes when failures is empty."""
    fails, ratios = [], {}
    worst = 0.0
    for key, p in energy_result.pairs.items():
        d = dev["residuals"][key]
        cand, en, dec = np.asarray(d["candidate"]), np.asarray(d["energy"]), p["decided"]
        bad = dec & (np.asarray(d["status"]) != p["status"])
        if bad.any():
            fails.append(f"{key}: status of decided items {np.flatnonzero(bad)[:8]}")
        bad = dec & (cand != p["candidate"])
        if bad.any():
            fails.append(f"{key}: candidate of decided items {np.flatnonzero(bad)[:8]}: {cand[bad][:8]} against {p['candidate'][bad][:8]}")
        und = ~dec
        if (und & ~np.isin(cand, (STATUS_OK, STATUS_OOB))).any():
            fails.append(f"{key}: candidate of undecided items is neither outcome")
        # the energy of the outcome the device took (decided items: the model's outcome)
        inside = np.where(dec, p["evaluate"], cand == STATUS_OK)
        diff = np.abs(en - np.where(inside, p["energy"].v, 0.0))
        bound = np.where(inside, p["energy"].e, 0.0)
        q = _ratio(diff, bound)
        worst = max(worst, q)
        if q > 1:
            i = int(np.argmax(np.where(diff > bound, diff, -1)))
            fails.append(f"{key}: energy of item {i}: {en[i]!r} against {float(np.where(inside, p['energy'].v, 0.0)[i])!r} +- {bound[i]:.3e}")
    ratios["residual energy"] = worst
    q = _ratio(dev["energy"] - energy_result.energy.v, energy_result.energy.e)
    ratios["total energy"] = q
    if q > 1:
        fails.append(f"total energy {dev['energy']!r} against {float(energy_result.energy.v)!r} +- {float(energy_result.energy.e):.3e}")
    if not energy_result.count[0] <= dev["count"] <= energy_result.count[1]:
        fails.append(f"valid count {dev['count']} outside {energy_result.count}")
    if lin_result is not None:
        F = len(lin_result.landmarks)
        for name, a, m in zip(("H_pp", "b_pp", "H_schur", "b_schur"), dev["system"], lin_result.system):
            q = _ratio(a - m.v, m.e)
            ratios[name] = q
            if q > 1:
                d = np.abs(a - m.v) - m.e
                i = np.unravel_index(int(np.argmax(d)), d.shape)
                fails.append(f"{name}{list(i)}: {a[i]!r} against {m.v[i]!r} +- {m.e[i]:.3e}")
        free = [k for r in range(F) for k in range(8 * r, 8 * r + 8) if lin_result.system[0].v[8 * r, 8 * r] < 1e15]
        sub = np.ix_(free, free)
        ratios["H_pp free"] = _ratio(dev["system"][0][sub] - lin_result.system[0].v[sub], lin_result.system[0].e[sub])
        if ratios["H_pp free"] > 1:
            fails.append("H_pp: free part")
        for name in ("hpib", "b_d", "inv_hdd"):
            worst = 0.0
            for r, lm in lin_result.landmarks.items():
                a, m = np.asarray(dev["landmarks"][r][name]), lm[name]
                q = _ratio(a - m.v, m.e)
                worst = max(worst, q)
                if q > 1:
                    d = np.abs(a - m.v) - m.e
                    i = np.unravel_index(int(np.argmax(d)), d.shape)
                    fails.append(f"{name} of keyframe {r}, landmark {list(i)}: {a[i]!r} against {m.v[i]!r} +- {m.e[i]:.3e}")
            ratios[name] = worst
    return fails, ratios


def unbounded(lin_result):
    """number of system and landmark entries the model gives no finite bound for (undecided items next to a vanishing H_dd)"""
    n = sum(int(np.isinf(x.e).sum()) for x in lin_result.system)
    return n + sum(int(np.isinf(np.broadcast_to(x.e, x.v.shape)).sum()) for lm in lin_result.landmarks.values() for x in lm.values())


def compare_opening(status, first, final):
    """statuses after optimize() with one iteration (the WFEJ opening sweep at the initial state, the step accepted): for items decided in
    both evaluations, the candidate of `final` - the residual-only sweep at the device's final state, whose first-estimate item test is
    that of `first` (FEJ linearisation at the initial state: same snapshot inverse depths, same linearisation point).
    Returns (failures, number of exempt items)."""
    fails, exempt = [], 0
    for key, pf in final.pairs.items():
        p0 = first.pairs[key]
        assert np.array_equal(p0["fej_ok"], pf["fej_ok"])
        dec = pf["decided"] & p0["decided"]
        exempt += int((~dec).sum())
        want = pf["candidate"]
        bad = dec & (np.asarray(status[key]) != want)
        if bad.any():
            fails.append(f"{key}: status of items {np.flatnonzero(bad)[:8]}: {np.asarray(status[key])[bad][:8]} against {want[bad][:8]}")
    return fails, exempt
