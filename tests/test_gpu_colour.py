"""Colour frames on the device (colour.hip, dsopp_hip_pyramid_build_colour, dsopp_hip_pyramid_get_image) against the NumPy model of
tests/colour_model.py, bit for bit: the arithmetic is integer, so there is no tolerance anywhere.  The sizes, maps and transformer cases
are those of test_gpu_undistort.py and test_gpu_transform.py, the smallest at which these kernels can go wrong: every N mod 4 of the
bytewise tail, rows that are no multiple of 4 bytes, more than one workgroup, several reflections (where a step of 1 instead of 3 bytes
shows), exact ties, upscales with clamped last taps, 2 x 2 inputs, the pure crop and nothing to do at all."""
import functools

import numpy as np
import pytest

import colour_model as cm
import semantics_model as sm
import test_gpu_semantics as tgs
import test_gpu_transform as tgt
import test_gpu_undistort as tgu
import transform_model as tm
import undistort_model as um

pytestmark = pytest.mark.gpu

ERR_INVALID_ARGUMENT = -1
MAPS = ("identity", "half_pixel", "simple_radial", "random", "ties")
SOURCES = ("random", "extreme", "equal")
GUARD = 0xA5


@functools.lru_cache(maxsize=None)
def _bgr(kind, W, H, seed=0):
    """random: any bytes; extreme: every channel byte 0 or 255 (the largest sums); equal: B = G = R (the grey path in three channels)"""
    rng = np.random.default_rng(W * 131 + H + len(kind) + 7919 * seed)
    if kind == "random":
        img = rng.integers(0, 256, (H, W, 3))
    elif kind == "extreme":
        img = rng.integers(0, 2, (H, W, 3)) * 255
    else:
        img = np.repeat(rng.integers(0, 256, (H, W, 1)), 3, axis=2)
    img = np.ascontiguousarray(img.astype(np.uint8))
    img.setflags(write=False)
    return img


def _check_stage(run, src, want_colour, want_grey, what, in_offset=0):
    """`run(in_ptr, bgr_out_ptr, grey_out_ptr, stream)` between torch buffers on a torch stream: colour only, grey only and both, each
    twice; the results equal the model, an output that was not asked for and the bytes behind each output stay untouched"""
    import torch
    n = want_grey.size
    d_in = torch.zeros(src.size + 8, dtype=torch.uint8, device="cuda")
    d_in[in_offset:in_offset + src.size] = torch.from_numpy(src.reshape(-1).copy()).cuda()
    stream = torch.cuda.Stream()
    for colour, grey in ((True, False), (False, True), (True, True)):
        d_bgr = torch.full((3 * n + 8,), GUARD, dtype=torch.uint8, device="cuda")
        d_grey = torch.full((n + 8,), GUARD, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        results = []
        for _ in range(2):
            run(d_in.data_ptr() + in_offset, d_bgr.data_ptr() if colour else None, d_grey.data_ptr() if grey else None, stream.cuda_stream)
            stream.synchronize()
            results.append((d_bgr.cpu().numpy(), d_grey.cpu().numpy()))
        got_bgr, got_grey = results[0]
        if colour:
            assert np.array_equal(got_bgr[:3 * n].reshape(want_colour.shape), want_colour), (what, colour, grey)
        if grey:
            assert np.array_equal(got_grey[:n].reshape(want_grey.shape), want_grey), (what, colour, grey)
        assert (got_bgr[3 * n if colour else 0:] == GUARD).all() and (got_grey[n if grey else 0:] == GUARD).all(), (what, colour, grey)
        assert np.array_equal(results[1][0], got_bgr) and np.array_equal(results[1][1], got_grey), (what, colour, grey)


# ---- the two stage forms and the plain conversion

@pytest.mark.parametrize("kind", MAPS)
@pytest.mark.parametrize("size", tgu.SIZES)
def test_undistort_bgr_device_matches_model(size, kind):
    from dsopp_amd import capi
    in_size, out_size = tgu.SIZES[size]
    maps = tgu._maps(kind, in_size, out_size)
    u = capi.Undistorter(in_size, out_size, *maps)
    try:
        for source in SOURCES:
            src = _bgr(source, *in_size)
            want_colour = cm.remap_bgr(src, *maps)
            want_grey = cm.bgr_to_grey(want_colour)
            if source == "equal":   # the colour path of a grey image is the existing grey kernel's output
                grey_kernel = u.undistort(np.ascontiguousarray(src[..., 0]))
                assert np.array_equal(want_grey, grey_kernel) and all(np.array_equal(want_colour[..., c], grey_kernel) for c in range(3))
            _check_stage(u.undistort_bgr_device, src, want_colour, want_grey, (size, kind, source))
    finally:
        u.close()


@pytest.mark.parametrize("case", tgt.CASES)
def test_transform_bgr_device_matches_model(case):
    in_size, ratio, levels, out_size = tgt.CASES[case]
    t = tgt._transformer(case)
    try:
        for source in SOURCES:
            src = _bgr(source, *in_size)
            want_colour = cm.transform_bgr(src, ratio, levels)
            want_grey = cm.bgr_to_grey(want_colour)
            assert want_grey.shape == (out_size[1], out_size[0])
            if source == "equal":
                grey_kernel = t.transform_image(np.ascontiguousarray(src[..., 0]))
                assert np.array_equal(want_grey, grey_kernel) and all(np.array_equal(want_colour[..., c], grey_kernel) for c in range(3))
            _check_stage(t.transform_bgr_device, src, want_colour, want_grey, (case, source))
    finally:
        t.close()


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_the_input_may_have_any_alignment(offset):
    """the frame starts `offset` bytes behind a word boundary: both stages, and the plain conversion of a transformer with nothing to do,
    whose kernel reads words only from an aligned input (65 x 45 and 66 x 45: with a bytewise tail, more than one workgroup)"""
    from dsopp_amd import capi
    in_size, out_size = tgu.SIZES["80x60to67x45"]
    maps = tgu._maps("random", in_size, out_size)
    u, t = capi.Undistorter(in_size, out_size, *maps), tgt._transformer("70x50_r0.91_c0")
    same = [capi.Transformer(size, 1.0, 0) for size in ((65, 45), (66, 45), (64, 48))]
    try:
        src = _bgr("random", *in_size)
        want = cm.remap_bgr(src, *maps)
        _check_stage(u.undistort_bgr_device, src, want, cm.bgr_to_grey(want), "remap", offset)
        src = _bgr("random", 70, 50)
        want = cm.transform_bgr(src, 0.91, 0)
        _check_stage(t.transform_bgr_device, src, want, cm.bgr_to_grey(want), "resize", offset)
        for s in same:
            src = _bgr("extreme", *s.in_size)
            _check_stage(s.transform_bgr_device, src, src, cm.bgr_to_grey(src), ("conversion", s.in_size), offset)
    finally:
        for h in (u, t, *same):
            h.close()


def test_stage_forms_on_their_own_streams():
    import torch
    from dsopp_amd import capi
    in_size, out_size = tgu.SIZES["80x60to67x45"]
    maps = tgu._maps("simple_radial", in_size, out_size)
    u, t = capi.Undistorter(in_size, out_size, *maps), tgt._transformer("80x60_r0.75_c4")
    try:
        src = _bgr("random", *in_size)
        d_in = torch.from_numpy(src.copy()).cuda()
        d_a, d_b = torch.zeros(67 * 45, dtype=torch.uint8, device="cuda"), torch.zeros(48 * 32, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        u.undistort_bgr_device(d_in.data_ptr(), None, d_a.data_ptr())
        t.transform_bgr_device(d_in.data_ptr(), None, d_b.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d_a.cpu().numpy().reshape(45, 67), cm.bgr_to_grey(cm.remap_bgr(src, *maps)))
        assert np.array_equal(d_b.cpu().numpy().reshape(32, 48), cm.frame(src, None, 0.75, 4)[1])
    finally:
        u.close()
        t.close()


# ---- the pyramid's colour build

LUT = 255.0 * (np.arange(256) / 255.0) ** 1.3 + 0.25
# the four rows of the launch table (and a transformer with nothing to do, which is the fourth again):
# (undistorter (size key, maps) or None, transformer case or None, levels)
BUILDS = {
    "remap+resize": (("64x48to80x60", "half_pixel"), "80x60_r0.75_c4", 3),
    "remap": (("80x60to67x45", "random"), None, 2),
    "resize": (None, "67x45_r1.5_c0", 2),
    "crop": (None, "70x50_r1_c4", 3),
    "conversion": (None, None, 3),
    "remap+nothing": (("64x48", "simple_radial"), "64x48_r1_c4", 3),
    "nothing": (None, "64x48_r1_c4", 3),
}
UNDISTORTER_SIZES = dict(tgu.SIZES, **{"64x48to80x60": ((64, 48), (80, 60))})


class _Chain:
    """the handles of one BUILDS row and the model of what they do to a frame"""

    def __init__(self, build):
        from dsopp_amd import capi
        undistorter, case, self.levels = BUILDS[build]
        self.u = self.t = self.maps = None
        self.ratio, self.crop = 1.0, 0
        self.in_size = self.out_size = (64, 48)
        if case is not None:
            self.in_size, self.ratio, self.crop, self.out_size = tgt.CASES[case]
            self.t = tgt._transformer(case)
        if undistorter is not None:
            size, kind = undistorter
            self.in_size, remapped = UNDISTORTER_SIZES[size]
            self.maps = tgu._maps(kind, self.in_size, remapped)
            self.u = capi.Undistorter(self.in_size, remapped, *self.maps)
            if case is None:
                self.out_size = remapped

    def model(self, bgr):
        return cm.frame(bgr, self.maps, self.ratio, self.crop)

    def close(self):
        for h in (self.u, self.t):
            if h is not None:
                h.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("build", BUILDS)
def test_build_colour_equals_build_of_the_model_grey_image(build, dtype):
    """three different frames through the same pyramid, the first with a LUT and a vignette: every level's texels equal those of a plain
    build of the model's grey image; get_image(1) is that image, get_image(3) the model's colour image when it was kept"""
    from dsopp_amd import capi
    c = _Chain(build)
    w, h = c.out_size
    F = capi.F64 if dtype == "f64" else capi.F32
    vig = np.random.default_rng(8).integers(90, 256, (h, w)).astype(np.uint8)
    a, b = capi.Pyramid(w, h, c.levels, F), capi.Pyramid(w, h, c.levels, F)
    try:
        assert a.get_image(1) is None and a.get_image(3) is None
        for seed, kind, lut, vignette, keep in ((1, "random", LUT, vig, True), (2, "extreme", None, None, False), (3, "random", None, None, True)):
            frame = _bgr(kind, *c.in_size, seed=seed)
            want_colour, want_grey = c.model(frame)
            assert want_grey.shape == (h, w)
            a.build_colour(c.u, c.t, frame, lut, vignette, keep_colour=keep)
            b.build(want_grey, lut, vignette)
            for level in range(c.levels):
                got, want = a.get_level(level), b.get_level(level)
                assert np.array_equal(got, want), (build, dtype, seed, level)
                assert np.abs(want[..., 1:]).max() > 0
            assert np.array_equal(a.get_image(1), want_grey), (build, dtype, seed)
            kept = a.get_image(3)
            assert (kept is None) if not keep else np.array_equal(kept, want_colour), (build, dtype, seed)
    finally:
        a.close()
        b.close()
        c.close()


def test_other_builds_drop_the_colour_image_and_get_image_follows_the_kept_grey_one():
    from dsopp_amd import capi
    c = _Chain("remap+resize")
    w, h = c.out_size
    grey_u = capi.Undistorter((80, 60), (80, 60), *tgu._maps("half_pixel", (80, 60), (80, 60)))
    p = capi.Pyramid(w, h, 2)
    try:
        frame = _bgr("random", *c.in_size)
        colour, grey = c.model(frame)
        p.build_colour(c.u, c.t, frame, keep_colour=True)
        assert np.array_equal(p.get_image(3), colour) and np.array_equal(p.get_image(1), grey)
        grey_frame = tgt._source("random", 80, 60)
        p.build_transformed(grey_u, c.t, grey_frame)       # a grey frame through the grey kernels
        assert p.get_image(3) is None
        assert np.array_equal(p.get_image(1), tm.transform_image(um.remap(grey_frame, *tgu._maps("half_pixel", (80, 60), (80, 60))), 0.75, 4))
        p.build_colour(c.u, c.t, frame, keep_colour=True)
        p.build(grey)                                      # a plain build keeps no 8-bit image at all
        assert p.get_image(3) is None and p.get_image(1) is None
        assert np.array_equal(p.get_level(0)[..., 0], grey.astype(np.float64))
    finally:
        p.close()
        grey_u.close()
        c.close()


# ---- the consumers of the kept grey image

def _colour_camera_frame(i):
    """three different channels of a rendered scene"""
    f = tgt._camera_frame(i)
    return np.ascontiguousarray(np.stack([f, np.roll(f, 9, axis=1), 255 - np.roll(f, 5, axis=0)], axis=-1))


def test_extract_from_pyramid_equals_extract_of_the_model_grey_image():
    """640 x 480 colour frames, remapped, at 0.75 and 4 crop levels = 480 x 352; two frames in a row (the second call adapts the state):
    lists and state as extract() of the model's grey image from the host"""
    from dsopp_amd import capi
    W, H = tgt.EX_W, tgt.EX_H
    maps = tgt._half_pixel_maps(W, H)
    t, u = capi.Transformer((W, H), 0.75, 4), capi.Undistorter((W, H), (W, H), *maps)
    w, h = t.out_size
    pyr = capi.Pyramid(w, h, 2, capi.F32)
    from_pyramid, from_host = capi.FeatureExtractor(w, h), capi.FeatureExtractor(w, h)
    try:
        for i in range(2):
            frame = _colour_camera_frame(i)
            _, grey = cm.frame(frame, maps, 0.75, 4)
            pyr.build_colour(u, t, frame)
            got, want = from_pyramid.extract_from_pyramid(pyr), from_host.extract(grey)
            assert len(want) > 50 and got.shape == want.shape and np.array_equal(got, want), (i, got.shape, want.shape)
            assert from_pyramid.state() == from_host.state(), i
    finally:
        for handle in (from_pyramid, from_host, pyr, t, u):
            handle.close()


def test_set_mask_from_pyramid_behind_a_colour_build():
    from dsopp_amd import capi
    W, H = 200, 136
    static, filt = np.full((H, W), 255, dtype=np.uint8), tgs._is_filtered()
    static[int(0.55 * H):int(0.55 * H) + 5, :] = 0
    from_pyramid, from_host = capi.FeatureExtractor(W, H, 300.0), capi.FeatureExtractor(W, H, 300.0)
    s = capi.Semantics(W, H, tgs.LEVELS, static, filt)
    p = capi.Pyramid(W, H, tgs.LEVELS)
    try:
        f = tgs._textured_frame(W, H, 0)
        frame = np.ascontiguousarray(np.stack([f, np.roll(f, 9, axis=1), 255 - f], axis=-1))
        cls = tgs._class_image(W, H, 30)
        p.build_colour(None, None, frame)
        p.set_semantics(s, cls)
        from_pyramid.set_mask_from_pyramid(p)
        got = from_pyramid.extract_from_pyramid(p, keep_mask=True)
        want = from_host.extract(cm.bgr_to_grey(frame), mask=sm.filter_mask(static, cls, filt))
        assert len(want) > 20 and got.shape == want.shape and np.array_equal(got, want), (got.shape, want.shape)
        assert from_pyramid.state() == from_host.state()
    finally:
        for handle in (from_pyramid, from_host, p, s):
            handle.close()


# ---- errors: each is DSOPP_HIP_ERR_INVALID_ARGUMENT and leaves the handles usable

def _refused(call, *args, **kw):
    from dsopp_amd import capi
    with pytest.raises(capi.HipError, match=f"error {ERR_INVALID_ARGUMENT}:"):
        call(*args, **kw)


def test_stage_argument_errors():
    import torch
    c = _Chain("remap+resize")
    try:
        src = _bgr("random", 64, 48)
        d_in = torch.from_numpy(src.copy()).cuda()
        d_bgr = torch.zeros(3 * 80 * 60 + 8, dtype=torch.uint8, device="cuda")
        d_grey = torch.zeros(80 * 60 + 8, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for run in (c.u.undistort_bgr_device, c.t.transform_bgr_device):
            _refused(run, None, d_bgr.data_ptr(), d_grey.data_ptr())              # no frame
            _refused(run, d_in.data_ptr(), None, None)                            # no output
            for off_bgr, off_grey in ((1, 0), (0, 2), (3, 3)):
                _refused(run, d_in.data_ptr(), d_bgr.data_ptr() + off_bgr, d_grey.data_ptr() + off_grey)
            _refused(run, d_in.data_ptr(), d_bgr.data_ptr() + 2, None)
            _refused(run, d_in.data_ptr(), None, d_grey.data_ptr() + 1)
        torch.cuda.synchronize()
        assert not d_bgr.any() and not d_grey.any()   # nothing was launched
        want = cm.remap_bgr(src, *c.maps)
        c.u.undistort_bgr_device(d_in.data_ptr(), d_bgr.data_ptr() + 4, d_grey.data_ptr() + 4)
        torch.cuda.synchronize()
        assert np.array_equal(d_bgr.cpu().numpy()[4:4 + want.size].reshape(want.shape), want)
        assert np.array_equal(d_grey.cpu().numpy()[4:4 + 80 * 60].reshape(60, 80), cm.bgr_to_grey(want))
    finally:
        c.close()


def test_build_and_getter_argument_errors():
    import ctypes as C
    from dsopp_amd import capi
    c = _Chain("remap+resize")                          # 64 x 48 -> 80 x 60 -> 48 x 32
    other_u = capi.Undistorter((80, 60), (67, 45), *tgu._maps("random", (80, 60), (67, 45)))
    wrong, right = capi.Pyramid(60, 45, 2), capi.Pyramid(48, 32, 2)
    try:
        frame = _bgr("random", 64, 48)
        null = capi.lib().dsopp_hip_pyramid_build_colour(right._h, c.u._h, c.t._h, None, None, None, 1)
        assert null == ERR_INVALID_ARGUMENT
        _refused(wrong.build_colour, c.u, c.t, frame)                             # the transformer writes 48 x 32
        _refused(right.build_colour, other_u, c.t, _bgr("random", 80, 60))        # the undistorter writes 67 x 45, the transformer reads 80 x 60
        _refused(right.build_colour, other_u, None, _bgr("random", 80, 60))       # the undistorter writes 67 x 45, the pyramid is 48 x 32
        _refused(wrong.build_colour, None, c.t, _bgr("random", 80, 60))
        assert right.get_image(1) is None and right.get_image(3) is None
        right.build_colour(c.u, c.t, frame, keep_colour=True)
        colour, grey = c.model(frame)
        out, present = np.full((32, 48, 2), GUARD, dtype=np.uint8), C.c_int(7)
        for channels in (2, 0, 4, -1):
            rc = capi.lib().dsopp_hip_pyramid_get_image(right._h, channels, out.ctypes.data_as(C.c_void_p), C.byref(present))
            assert rc == ERR_INVALID_ARGUMENT and present.value == 7 and (out == GUARD).all(), channels
        assert np.array_equal(right.get_image(3), colour) and np.array_equal(right.get_image(1), grey)
        wrong.build(tgt._source("random", 60, 45))      # the refused pyramid still builds
        assert wrong.get_level(0)[..., 0].max() == tgt._source("random", 60, 45).max()
    finally:
        for handle in (wrong, right, other_u):
            handle.close()
        c.close()
