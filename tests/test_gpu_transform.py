"""The device image transformer (dsopp_hip_transformer, transform.hip), the pyramid's transformed build, the extractor's read of its
kept image and the transformed semantics path against the NumPy model of tests/transform_model.py, bit for bit: the arithmetic is
integer, so there is no tolerance anywhere.  The sizes are the smallest at which the kernel can go wrong: every N mod 4 of the bytewise
tail, rows that are no multiple of 4 bytes (a thread's word then spans two rows), more than one workgroup, an upscale whose last column
and row clamp, a 2 x 2 input where every tap clamps, the pure crop, and nothing to do at all.  The ratios keep size * ratio away from
integers, so the truncation of the sizes is no rounding coin-flip."""
import functools

import numpy as np
import pytest

import semantics_model as sm
import transform_model as tm
import undistort_model as um

pytestmark = pytest.mark.gpu

ERR_INVALID_ARGUMENT = -1
LINEAR, NEAREST = 0, 1
# input (width, height), ratio, crop levels, output (width, height)
CASES = {
    "80x60_r0.75_c4": ((80, 60), 0.75, 4, (48, 32)),     # via 60 x 45: crop in both axes, 384 words
    "67x45_r1.5_c0": ((67, 45), 1.5, 0, (100, 67)),      # upscale, clamped last column and row
    "65x45_r0.61_c0": ((65, 45), 0.61, 0, (39, 27)),     # 1053 bytes = 1 mod 4
    "71x47_r0.9_c0": ((71, 47), 0.9, 0, (63, 42)),       # 2646 bytes = 2 mod 4
    "70x50_r0.91_c0": ((70, 50), 0.91, 0, (63, 45)),     # 2835 bytes = 3 mod 4
    "2x2_r1.5_c0": ((2, 2), 1.5, 0, (3, 3)),             # smallest input, every clamp
    "32x32_r0.5_c4": ((32, 32), 0.5, 4, (16, 16)),       # the 2 x 2 mean
    "70x50_r1_c4": ((70, 50), 1.0, 4, (64, 48)),         # pure crop
    "64x48_r1_c4": ((64, 48), 1.0, 4, (64, 48)),         # nothing to do
}
KINDS = ("random", "extreme", "classes")


@functools.lru_cache(maxsize=None)
def _source(kind, W, H):
    rng = np.random.default_rng(W * 131 + H + len(kind))
    if kind == "random":
        img = rng.integers(0, 256, (H, W))
    elif kind == "extreme":
        img = rng.integers(0, 2, (H, W)) * 255
    else:
        img = rng.integers(0, 9, (H, W)) * 31
    img = img.astype(np.uint8)
    img.setflags(write=False)
    return img


def _interpolation(kind):
    return NEAREST if kind == "classes" else LINEAR


@functools.lru_cache(maxsize=None)
def _expected(kind, case):
    in_size, ratio, levels, out_size = CASES[case]
    model = tm.transform_mask if kind == "classes" else tm.transform_image
    out = model(_source(kind, *in_size), ratio, levels)
    assert out.shape == (out_size[1], out_size[0]), out.shape
    out.setflags(write=False)
    return out


def _transformer(case, **kw):
    from dsopp_amd import capi
    in_size, ratio, levels, _ = CASES[case]
    return capi.Transformer(in_size, ratio, levels, **kw)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES)
def test_transform_matches_model(case, kind):
    """the blocking host form, twice: both results equal the model"""
    in_size, ratio, levels, out_size = CASES[case]
    t = _transformer(case)
    try:
        assert t.sizes() == (in_size, tm.sizes(in_size, ratio, levels)[0], out_size) and t.out_size == out_size
        src, want = _source(kind, *in_size), _expected(kind, case)
        run = t.transform_mask if kind == "classes" else t.transform_image
        first, second = run(src), run(src)
        assert np.array_equal(first, want), (case, kind, int((first != want).sum()))
        assert np.array_equal(second, first)
    finally:
        t.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES)
def test_transform_device_matches_model(case, kind):
    """the enqueue-only form between torch-allocated buffers on a torch stream, twice; the bytes behind the output stay untouched"""
    import torch
    t = _transformer(case)
    try:
        src, want = _source(kind, *CASES[case][0]), _expected(kind, case)
        n = want.size
        d_in = torch.from_numpy(src.copy()).cuda()
        d_out = torch.full((n + 8,), 0xA5, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        results = []
        for _ in range(2):
            t.transform_device(d_in.data_ptr(), d_out.data_ptr(), _interpolation(kind), stream=stream.cuda_stream)
            stream.synchronize()
            results.append(d_out.cpu().numpy())
        assert np.array_equal(results[0][:n].reshape(want.shape), want), (case, kind)
        assert (results[0][n:] == 0xA5).all()
        assert np.array_equal(results[1], results[0])
    finally:
        t.close()


def test_transform_device_on_its_own_stream():
    import torch
    case = "71x47_r0.9_c0"
    t = _transformer(case)
    try:
        want = _expected("random", case)
        d_in = torch.from_numpy(_source("random", 71, 47).copy()).cuda()
        d_out = torch.zeros(want.size, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        t.transform_device(d_in.data_ptr(), d_out.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d_out.cpu().numpy().reshape(want.shape), want)
    finally:
        t.close()


def test_the_two_interpolations_differ_and_the_closed_forms_hold_on_the_device():
    t = _transformer("32x32_r0.5_c4")
    try:
        src = _source("random", 32, 32)
        p = src.astype(np.int64)
        mean = ((p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2).astype(np.uint8)
        assert np.array_equal(t.transform_image(src), mean) and np.array_equal(t.transform_mask(src), src[0::2, 0::2])
        assert not np.array_equal(mean, src[0::2, 0::2])
    finally:
        t.close()
    t = _transformer("70x50_r1_c4")
    try:
        src = _source("random", 70, 50)
        assert np.array_equal(t.transform_image(src), src[:48, :64]) and np.array_equal(t.transform_mask(src), src[:48, :64])
    finally:
        t.close()


# ---- the pyramid's transformed build

LUT = 255.0 * (np.arange(256) / 255.0) ** 1.3 + 0.25
PYRAMIDS = {"48x32x3": ("80x60_r0.75_c4", 3), "100x67x2": ("67x45_r1.5_c0", 2), "crop64x48x3": ("70x50_r1_c4", 3), "same64x48x3": ("64x48_r1_c4", 3)}


@functools.lru_cache(maxsize=None)
def _half_pixel_maps(w, h):
    mx, my = um.identity_maps(w, h)
    mx, my = mx + np.float32(0.5), my + np.float32(0.5)
    for m in (mx, my):
        m.setflags(write=False)
    return mx, my


@functools.lru_cache(maxsize=None)
def _expected_frame(case, undistorted, seed):
    """the image the levels are built from: the model's remap (if any), then the model's resize and crop"""
    in_size, ratio, levels, _ = CASES[case]
    frame = np.random.default_rng(seed).integers(0, 256, (in_size[1], in_size[0])).astype(np.uint8)
    image = um.remap(frame, *_half_pixel_maps(*in_size)) if undistorted else frame
    out = tm.transform_image(image, ratio, levels)
    for a in (frame, out):
        a.setflags(write=False)
    return frame, out


@pytest.mark.parametrize("undistorted", [True, False], ids=["remap", "noremap"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape", PYRAMIDS)
def test_build_transformed_equals_build_of_the_model_image(shape, dtype, undistorted):
    """three frames through the same pyramid, the first with LUT and vignette (level by level), the others without a vignette (all levels
    in one launch): every level's texels equal those of a plain build of the model's image"""
    from dsopp_amd import capi
    case, levels = PYRAMIDS[shape]
    in_size, _, _, (w, h) = CASES[case]
    F = capi.F64 if dtype == "f64" else capi.F32
    vig = np.random.default_rng(8).integers(90, 256, (h, w)).astype(np.uint8)
    u = capi.Undistorter(in_size, in_size, *_half_pixel_maps(*in_size)) if undistorted else None
    t = _transformer(case)
    a, b = capi.Pyramid(w, h, levels, F), capi.Pyramid(w, h, levels, F)
    try:
        for seed, lut, vignette in ((21, LUT, vig), (22, None, None), (23, LUT, None)):
            frame, want_image = _expected_frame(case, undistorted, seed)
            a.build_transformed(u, t, frame, lut, vignette)
            b.build(want_image, lut, vignette)
            for level in range(levels):
                got, want = a.get_level(level), b.get_level(level)
                assert np.array_equal(got, want), (shape, dtype, undistorted, seed, level)
                assert np.abs(want[..., 1:]).max() > 0
    finally:
        a.close()
        b.close()
        t.close()
        if u is not None:
            u.close()


# ---- the extractor's read of the pyramid's transformed image

EX_W, EX_H = 640, 480


@functools.lru_cache(maxsize=None)
def _camera_frame(i):
    """frame i of a short camera path through a rendered scene, as u8: here the image the camera delivers"""
    from dsopp_amd import synthetic as syn
    T = syn.se3_exp(np.array([0.03 * i, -0.01 * i, 0.02 * i, 0.002 * i, -0.003 * i, 0.001 * i]))
    img, _ = syn.Scene.make(EX_W, EX_H, seed=11).render_torch(T, 0.02 * i, 1.5 * i, "cuda")
    return np.clip(np.round(img), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("undistorted", [True, False], ids=["remap", "noremap"])
def test_extract_from_pyramid_equals_extract_of_the_model_image(undistorted):
    """640 x 480 at 0.75 and 4 crop levels = 480 x 352; two frames in a row (the second call adapts the state): lists and state as
    extract() of the model's image from the host"""
    from dsopp_amd import capi
    t = capi.Transformer((EX_W, EX_H), 0.75, 4)
    w, h = t.out_size
    assert (w, h) == (480, 352)
    u = capi.Undistorter((EX_W, EX_H), (EX_W, EX_H), *_half_pixel_maps(EX_W, EX_H)) if undistorted else None
    pyr = capi.Pyramid(w, h, 2, capi.F32)
    from_pyramid, from_host = capi.FeatureExtractor(w, h), capi.FeatureExtractor(w, h)
    try:
        for i in range(2):
            frame = _camera_frame(i)
            image = tm.transform_image(um.remap(frame, *_half_pixel_maps(EX_W, EX_H)) if undistorted else frame, 0.75, 4)
            pyr.build_transformed(u, t, frame)
            got, want = from_pyramid.extract_from_pyramid(pyr), from_host.extract(image)
            assert len(want) > 50 and got.shape == want.shape and np.array_equal(got, want), (i, got.shape, want.shape)
            assert from_pyramid.state() == from_host.state(), i
    finally:
        from_pyramid.close()
        from_host.close()
        pyr.close()
        t.close()
        if u is not None:
            u.close()


# ---- semantics behind a transformer

LEVELS = 4
# class image (width, height), ratio, crop levels, masks (width, height): one workgroup per level, and several
SEMANTICS = {"80x60to48x32": ((80, 60), 0.75, 4, (48, 32)), "230x150to192x128": ((230, 150), 0.9, 4, (192, 128))}


@functools.lru_cache(maxsize=None)
def _class_image(W, H, seed):
    """piecewise constant over 6 classes in blocks of 7 x 5 pixels"""
    rng = np.random.default_rng(seed)
    blocks = rng.integers(0, 6, ((H + 4) // 5, (W + 6) // 7)).astype(np.uint8)
    img = np.ascontiguousarray(np.kron(blocks, np.ones((5, 7), dtype=np.uint8))[:H, :W])
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _raw_static_mask(W, H):
    rng = np.random.default_rng(W + 7 * H)
    m = np.full((H, W), 255, dtype=np.uint8)
    m[int(0.55 * H):int(0.55 * H) + 7, :] = 0
    m[rng.random((H, W)) < 0.15] = 0
    m.setflags(write=False)
    return m


@pytest.mark.parametrize("undistorted", [True, False], ids=["remap", "noremap"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape", SEMANTICS)
def test_transformed_semantics_keep_the_model_class_image_and_masks(shape, dtype, undistorted):
    """class image -> remap -> nearest resize -> crop is what the pyramid keeps; the masks of every level are semantics_model's from the
    transformed static mask and that class image; two frames"""
    from dsopp_amd import capi
    in_size, ratio, crop, (w, h) = SEMANTICS[shape]
    maps = _half_pixel_maps(*in_size)
    filt = np.zeros(256, dtype=np.uint8)
    filt[[1, 4]] = (1, 200)
    u = capi.Undistorter(in_size, in_size, *maps) if undistorted else None
    t = capi.Transformer(in_size, ratio, crop)
    raw = _raw_static_mask(*in_size)
    # the once-per-camera path (camera_fabric.cpp:164): undistort, then runMaskTransformers
    static = t.transform_mask(u.undistort(raw) if undistorted else raw)
    assert np.array_equal(static, tm.transform_mask(um.remap(raw, *maps) if undistorted else raw, ratio, crop))
    s = capi.Semantics.transformed(t, LEVELS, static, filt, undistorter=u)
    p = capi.Pyramid(w, h, LEVELS, capi.F64 if dtype == "f64" else capi.F32)
    try:
        assert (s.width, s.height) == (w, h) and s.class_image_shape() == (in_size[1], in_size[0])
        p.build(np.random.default_rng(3).integers(0, 256, (h, w)).astype(np.uint8))
        texels = [p.get_level(l) for l in range(LEVELS)]
        seen = []
        for seed in (1, 2):
            raw_cls = _class_image(in_size[0], in_size[1], seed)
            cls = tm.transform_mask(um.remap(raw_cls, *maps) if undistorted else raw_cls, ratio, crop)
            p.set_semantics(s, raw_cls)
            assert np.array_equal(p.get_semantics(), cls), (shape, seed)
            valid, _ = sm.mask_pyramid(static, cls, filt, LEVELS)
            for l in range(LEVELS):
                got = p.get_mask(l)
                assert got.shape == valid[l].shape and np.array_equal(got, valid[l]), (shape, seed, l, int((got != valid[l]).sum()))
            assert 0 < valid[0].sum() < valid[0].size
            seen.append(valid[0])
            assert all(np.array_equal(p.get_level(l), texels[l]) for l in range(LEVELS))   # the other lanes stay
        assert not np.array_equal(seen[0], seen[1])     # the class image matters
        p.set_semantics(s, None)
        assert p.get_semantics() is None
        assert np.array_equal(p.get_mask(0), (static != 0).astype(np.uint8))
    finally:
        p.close()
        s.close()
        t.close()
        if u is not None:
            u.close()


# ---- errors: each leaves the handles usable

def _raw_create(in_size, ratio, levels, device=0):
    import ctypes as C
    from dsopp_amd import capi
    h = C.c_void_p()
    rc = capi.lib().dsopp_hip_transformer_create(device, None, in_size[0], in_size[1], C.c_double(ratio), levels, C.byref(h))
    assert rc != 0 and not h.value
    return rc


def test_create_errors_then_a_good_create_works():
    from dsopp_amd import capi
    for ratio in (float("nan"), float("inf"), 0.0, -0.75):
        assert _raw_create((64, 48), ratio, 4) == ERR_INVALID_ARGUMENT
    assert _raw_create((64, 48), 0.2, 4) == ERR_INVALID_ARGUMENT          # 12 x 9 crops to nothing
    assert _raw_create((64, 48), 1.0, 9) == ERR_INVALID_ARGUMENT
    assert _raw_create((0, 48), 1.0, 4) == ERR_INVALID_ARGUMENT
    assert _raw_create((64, 48), 0.75, 4, device=capi.device_count()) == ERR_INVALID_ARGUMENT
    t = _transformer("80x60_r0.75_c4")
    try:
        assert np.array_equal(t.transform_image(_source("random", 80, 60)), _expected("random", "80x60_r0.75_c4"))
    finally:
        t.close()


def test_misaligned_pointers_and_unknown_interpolations_are_refused():
    import torch
    from dsopp_amd import capi
    case = "80x60_r0.75_c4"
    t = _transformer(case)
    try:
        want = _expected("random", case)
        d_in = torch.zeros(80 * 60 + 8, dtype=torch.uint8, device="cuda")
        d_in[:80 * 60] = torch.from_numpy(_source("random", 80, 60).copy().reshape(-1)).cuda()
        d_out = torch.zeros(want.size + 8, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for off_in, off_out, interpolation in ((1, 0, LINEAR), (0, 2, LINEAR), (3, 3, NEAREST), (0, 0, 2), (0, 0, -1)):
            with pytest.raises(capi.HipError) as e:
                t.transform_device(d_in.data_ptr() + off_in, d_out.data_ptr() + off_out, interpolation)
            assert "-1" in str(e.value)
        torch.cuda.synchronize()
        assert not d_out.any()   # nothing was launched
        t.transform_device(d_in.data_ptr(), d_out.data_ptr() + 4)
        torch.cuda.synchronize()
        assert np.array_equal(d_out.cpu().numpy()[4:4 + want.size].reshape(want.shape), want)
    finally:
        t.close()


def test_mismatched_sizes_are_refused_and_everything_stays_usable():
    from dsopp_amd import capi
    case = "80x60_r0.75_c4"
    t = _transformer(case)
    fits, other = capi.Undistorter((80, 60), (80, 60)), capi.Undistorter((80, 60), (67, 45), *[m[:45, :67] for m in _half_pixel_maps(80, 60)])
    wrong, right = capi.Pyramid(60, 45, 2), capi.Pyramid(48, 32, 2)
    try:
        frame = _source("random", 80, 60)
        for pyramid, undistorter in ((wrong, None), (wrong, fits), (right, other)):
            with pytest.raises(capi.HipError) as e:
                pyramid.build_transformed(undistorter, t, frame)
            assert "-1" in str(e.value)
        with pytest.raises(capi.HipError) as e:      # the undistorter must write what the transformer reads
            capi.Semantics.transformed(t, 2, undistorter=other)
        assert "-1" in str(e.value)
        uncropped = _transformer("67x45_r1.5_c0")    # 100 x 67: no second level without a crop
        try:
            with pytest.raises(capi.HipError) as e:
                capi.Semantics.transformed(uncropped, 2)
            assert "-1" in str(e.value)
        finally:
            uncropped.close()
        wrong.build(_source("random", 60, 45))       # the pyramid still builds
        assert wrong.get_level(0)[..., 0].max() == _source("random", 60, 45).max()
        right.build_transformed(fits, t, frame)      # the identity undistorter: the transformer alone
        assert np.array_equal(right.get_level(0)[..., 0], _expected("random", case).astype(np.float64))
    finally:
        wrong.close()
        right.close()
        fits.close()
        other.close()
        t.close()


def test_another_device_is_refused():
    """handles on two devices when there are two; the device id behind the last one is refused at create either way"""
    from dsopp_amd import capi
    n = capi.device_count()
    with pytest.raises(capi.HipError) as e:
        capi.Transformer((80, 60), 0.75, 4, device=n)
    assert "-1" in str(e.value)
    t = _transformer("80x60_r0.75_c4")
    try:
        with pytest.raises(capi.HipError) as e:
            capi.Semantics.transformed(t, 2, device=n)
        assert "-1" in str(e.value)
        if n > 1:
            elsewhere = capi.Pyramid(48, 32, 2, device=1)
            try:
                with pytest.raises(capi.HipError) as e:
                    elsewhere.build_transformed(None, t, _source("random", 80, 60))
                assert "-1" in str(e.value)
                with pytest.raises(capi.HipError) as e:
                    capi.Semantics.transformed(t, 2, device=1)
                assert "-1" in str(e.value)
            finally:
                elsewhere.close()
    finally:
        t.close()
