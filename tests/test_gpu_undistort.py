"""The device undistorter (dsopp_hip_undistorter, undistort.hip), the pyramid's undistorted build and the extractors' read of its kept
image against the NumPy model of tests/undistort_model.py, bit for bit: the arithmetic is integer, so there is no tolerance anywhere.
The sizes are the smallest at which the kernel can go wrong: every N mod 4 of the bytewise tail, more than one workgroup (N = 3015
output bytes), different input and output sizes, and a 2 x 2 input where every tap reflects."""
import functools

import numpy as np
import pytest

import undistort_model as um

pytestmark = pytest.mark.gpu

# (input, output) as (width, height)
SIZES = {"64x48": ((64, 48), (64, 48)), "80x60to67x45": ((80, 60), (67, 45)), "66x45": ((66, 45), (66, 45)), "65x45": ((65, 45), (65, 45)),
         "2x2to5x3": ((2, 2), (5, 3))}
MAPS = ("identity", "half_pixel", "simple_radial", "tum_fov", "random", "ties")
ERR_INVALID_ARGUMENT = -1


@functools.lru_cache(maxsize=None)
def _source(W, H):
    img = np.random.default_rng(W * 131 + H).integers(0, 256, (H, W)).astype(np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _maps(kind, in_size, out_size):
    """float32 maps of the output's shape holding input coordinates"""
    (W, H), (w, h) = in_size, out_size
    if kind == "identity":
        mx, my = um.identity_maps(w, h)
    elif kind == "half_pixel":
        mx, my = um.identity_maps(w, h)
        mx, my = mx + np.float32(0.5), my + np.float32(0.5)
    elif kind == "simple_radial":   # the reference builds them with out == in; the coordinates are then stretched onto the input
        mx, my = um.simple_radial_maps(w, h, 0.8 * w, 0.49 * w, 0.51 * h, -0.25, 0.06)
        mx, my = _stretch(mx, W / w), _stretch(my, H / h)
    elif kind == "tum_fov":
        mx, my = um.tum_fov_maps(w, h, 0.7 * w, 0.72 * h, 0.51 * w, 0.48 * h, 0.93)
        mx, my = _stretch(mx, W / w), _stretch(my, H / h)
    elif kind == "random":          # several periods beyond both edges: multiple reflections
        rng = np.random.default_rng(w * 7 + W)
        mx = rng.uniform(-3 * W, 4 * W, (h, w)).astype(np.float32)
        my = rng.uniform(-3 * H, 4 * H, (h, w)).astype(np.float32)
    else:                           # every coordinate an exact tie (k + 0.5) / 32, on both sides of zero and of the far edge
        kx = np.arange(w)[None, :] * 37 + np.arange(h)[:, None] * 11 - 200
        ky = np.arange(w)[None, :] * 5 + np.arange(h)[:, None] * 41 - 150
        mx, my = ((kx + 0.5) / 32).astype(np.float32), ((ky + 0.5) / 32).astype(np.float32)
        assert np.array_equal(mx.astype(np.float64) * 32, kx + 0.5) and np.array_equal(my.astype(np.float64) * 32, ky + 0.5)
    for m in (mx, my):
        m.setflags(write=False)
    return mx, my


def _stretch(m, factor):
    """scale the coordinates that did not fail (the failure marker stays -1)"""
    return np.where(m == -1, m, m * np.float32(factor)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _expected(kind, size):
    in_size, out_size = SIZES[size]
    out = um.remap(_source(*in_size), *_maps(kind, in_size, out_size))
    out.setflags(write=False)
    return out


def _undistorter(kind, size, **kw):
    from dsopp_amd import capi
    in_size, out_size = SIZES[size]
    return capi.Undistorter(in_size, out_size, *_maps(kind, in_size, out_size), **kw)


@pytest.mark.parametrize("kind", MAPS)
@pytest.mark.parametrize("size", SIZES)
def test_undistort_matches_model(size, kind):
    """the blocking host form, twice: both results equal the model"""
    u = _undistorter(kind, size)
    try:
        assert u.sizes() == SIZES[size]
        src, want = _source(*SIZES[size][0]), _expected(kind, size)
        first, second = u.undistort(src), u.undistort(src)
        assert np.array_equal(first, want), (size, kind, int((first != want).sum()))
        assert np.array_equal(second, first)
    finally:
        u.close()


@pytest.mark.parametrize("kind", MAPS)
@pytest.mark.parametrize("size", SIZES)
def test_undistort_device_matches_model(size, kind):
    """the enqueue-only form between torch-allocated buffers on a torch stream, twice; the bytes behind the output stay untouched"""
    import torch
    u = _undistorter(kind, size)
    try:
        src, want = _source(*SIZES[size][0]), _expected(kind, size)
        n = want.size
        d_in = torch.from_numpy(src.copy()).cuda()
        d_out = torch.full((n + 8,), 0xA5, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        results = []
        for _ in range(2):
            u.undistort_device(d_in.data_ptr(), d_out.data_ptr(), stream=stream.cuda_stream)
            stream.synchronize()
            results.append(d_out.cpu().numpy())
        assert np.array_equal(results[0][:n].reshape(want.shape), want), (size, kind)
        assert (results[0][n:] == 0xA5).all()
        assert np.array_equal(results[1], results[0])
    finally:
        u.close()


def test_undistort_device_on_its_own_stream():
    import torch
    u = _undistorter("random", "80x60to67x45")
    try:
        want = _expected("random", "80x60to67x45")
        d_in = torch.from_numpy(_source(80, 60).copy()).cuda()
        d_out = torch.zeros(want.size, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        u.undistort_device(d_in.data_ptr(), d_out.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d_out.cpu().numpy().reshape(want.shape), want)
    finally:
        u.close()


@pytest.mark.parametrize("size", ["64x48", "66x45", "65x45"])
def test_no_maps_is_the_identity(size):
    from dsopp_amd import capi
    in_size, _ = SIZES[size]
    u = capi.Undistorter(in_size, in_size)
    try:
        src = _source(*in_size)
        assert np.array_equal(u.undistort(src), src)
    finally:
        u.close()


def test_failure_marker_reads_pixel_1_1():
    from dsopp_amd import capi
    marker = np.full((48, 64), -1, dtype=np.float32)
    u = capi.Undistorter((64, 48), (64, 48), marker, marker)
    try:
        src = _source(64, 48)
        assert (u.undistort(src) == src[1, 1]).all()
    finally:
        u.close()


# ---- the pyramid's undistorted build

LUT = 255.0 * (np.arange(256) / 255.0) ** 1.3 + 0.25
PYRAMIDS = {"67x45x2": ("80x60to67x45", "random", 2), "64x48x3": ("64x48", "simple_radial", 3)}


@pytest.mark.parametrize("vignette", [False, True], ids=["novig", "vig"])
@pytest.mark.parametrize("lut", [False, True], ids=["nolut", "lut"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape", PYRAMIDS)
def test_build_undistorted_equals_build_of_the_model_image(shape, dtype, lut, vignette):
    from dsopp_amd import capi
    size, kind, levels = PYRAMIDS[shape]
    (in_size, (w, h)) = SIZES[size]
    F = capi.F64 if dtype == "f64" else capi.F32
    vig = np.random.default_rng(8).integers(90, 256, (h, w)).astype(np.uint8) if vignette else None
    u = _undistorter(kind, size)
    a, b = capi.Pyramid(w, h, levels, F), capi.Pyramid(w, h, levels, F)
    try:
        for _ in range(2):   # the second build reuses the pyramid's buffers
            a.build_undistorted(u, _source(*in_size), LUT if lut else None, vig)
            b.build(_expected(kind, size), LUT if lut else None, vig)
            for level in range(levels):
                got, want = a.get_level(level), b.get_level(level)
                assert np.array_equal(got, want), (shape, dtype, lut, vignette, level)
                assert np.abs(want[..., 1:]).max() > 0
    finally:
        a.close()
        b.close()
        u.close()


# ---- the extractors' read of the pyramid's undistorted image

EX_W, EX_H = 640, 480


@functools.lru_cache(maxsize=None)
def _camera_frame(i):
    """frame i of a short camera path through a rendered scene, as u8: here the image the distorted camera delivers"""
    from dsopp_amd import synthetic as syn
    T = syn.se3_exp(np.array([0.03 * i, -0.01 * i, 0.02 * i, 0.002 * i, -0.003 * i, 0.001 * i]))
    img, _ = syn.Scene.make(EX_W, EX_H, seed=11).render_torch(T, 0.02 * i, 1.5 * i, "cuda")
    return np.clip(np.round(img), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _camera_maps():
    return um.tum_fov_maps(EX_W, EX_H, 0.7 * EX_W, 0.72 * EX_H, 0.51 * EX_W, 0.48 * EX_H, 0.93)


@pytest.mark.parametrize("kind", ["sobel", "eigen"])
def test_extract_from_pyramid_equals_extract_of_the_model_image(kind):
    """two frames in a row (the second call adapts the state): lists and state as extract() of the model's image from the host"""
    from dsopp_amd import capi
    u = capi.Undistorter((EX_W, EX_H), (EX_W, EX_H), *_camera_maps())
    pyr = capi.Pyramid(EX_W, EX_H, 2, capi.F32)
    from_pyramid, from_host = _extractor(kind), _extractor(kind)
    try:
        for i in range(2):
            distorted = _camera_frame(i)
            undistorted = um.remap(distorted, *_camera_maps())
            pyr.build_undistorted(u, distorted)
            got, want = from_pyramid.extract_from_pyramid(pyr), from_host.extract(undistorted)
            assert len(want) > 100 and got.shape == want.shape and np.array_equal(got, want), (kind, i, got.shape, want.shape)
            assert from_pyramid.state() == from_host.state(), (kind, i)
            if kind == "eigen":
                assert from_pyramid.stats() == from_host.stats(), i
        # the distortion matters: the distorted frame itself gives another list
        assert not np.array_equal(_first_list(kind, _camera_frame(0)), _first_list(kind, um.remap(_camera_frame(0), *_camera_maps())))
    finally:
        from_pyramid.close()
        from_host.close()
        pyr.close()
        u.close()


def _extractor(kind):
    from dsopp_amd import capi
    return capi.FeatureExtractor(EX_W, EX_H) if kind == "sobel" else capi.EigenFeatureExtractor(EX_W, EX_H, 1500.0)


def _first_list(kind, image):
    """the first extract() of a fresh extractor"""
    ex = _extractor(kind)
    try:
        return ex.extract(image)
    finally:
        ex.close()


# ---- errors: each leaves the handles usable

def _raw_create(in_size, out_size, map_x, map_y):
    import ctypes as C
    from dsopp_amd import capi
    h = C.c_void_p()
    ptr = lambda m: None if m is None else m.ctypes.data_as(C.c_void_p)
    rc = capi.lib().dsopp_hip_undistorter_create(0, None, in_size[0], in_size[1], out_size[0], out_size[1], ptr(map_x), ptr(map_y), C.byref(h))
    assert rc != 0 and not h.value
    return rc


def test_create_errors_then_a_good_create_works():
    mx, my = _maps("half_pixel", (64, 48), (64, 48))
    nan = mx.copy()
    nan[47, 63] = np.nan
    assert _raw_create((64, 48), (64, 48), nan, my) == ERR_INVALID_ARGUMENT
    assert _raw_create((64, 48), (64, 48), mx, nan) == ERR_INVALID_ARGUMENT
    assert _raw_create((64, 48), (64, 48), mx, None) == ERR_INVALID_ARGUMENT
    assert _raw_create((64, 48), (64, 48), None, my) == ERR_INVALID_ARGUMENT
    assert _raw_create((1, 48), (64, 48), mx, my) == ERR_INVALID_ARGUMENT
    u = _undistorter("half_pixel", "64x48")
    try:
        assert np.array_equal(u.undistort(_source(64, 48)), _expected("half_pixel", "64x48"))
    finally:
        u.close()


def test_misaligned_device_pointers_are_refused():
    import torch
    from dsopp_amd import capi
    u = _undistorter("half_pixel", "64x48")
    try:
        want = _expected("half_pixel", "64x48")
        d_in = torch.zeros(want.size + 8, dtype=torch.uint8, device="cuda")
        d_in[:want.size] = torch.from_numpy(_source(64, 48).copy().reshape(-1)).cuda()
        d_out = torch.zeros(want.size + 8, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for off_in, off_out in ((1, 0), (0, 2), (3, 3)):
            with pytest.raises(capi.HipError) as e:
                u.undistort_device(d_in.data_ptr() + off_in, d_out.data_ptr() + off_out)
            assert "-1" in str(e.value)
        torch.cuda.synchronize()
        assert not d_out.any()   # nothing was launched
        u.undistort_device(d_in.data_ptr(), d_out.data_ptr() + 4)
        torch.cuda.synchronize()
        assert np.array_equal(d_out.cpu().numpy()[4:4 + want.size].reshape(want.shape), want)
    finally:
        u.close()


def test_pyramid_size_mismatch_is_refused_and_both_stay_usable():
    from dsopp_amd import capi
    u = _undistorter("random", "80x60to67x45")
    wrong, right = capi.Pyramid(80, 60, 2), capi.Pyramid(67, 45, 2)
    try:
        with pytest.raises(capi.HipError) as e:
            wrong.build_undistorted(u, _source(80, 60))
        assert "-1" in str(e.value)
        wrong.build(_source(80, 60))     # the pyramid still builds
        assert wrong.get_level(0)[..., 0].max() == _source(80, 60).max()
        right.build_undistorted(u, _source(80, 60))
        assert np.array_equal(right.get_level(0)[..., 0], _expected("random", "80x60to67x45").astype(np.float64))
    finally:
        wrong.close()
        right.close()
        u.close()


@pytest.mark.parametrize("kind", ["sobel", "eigen"])
def test_extract_from_a_plainly_built_pyramid_is_refused(kind):
    from dsopp_amd import capi
    ex = _extractor(kind)
    u = capi.Undistorter((EX_W, EX_H), (EX_W, EX_H))
    pyr = capi.Pyramid(EX_W, EX_H, 1)
    try:
        img = _camera_frame(0)
        before = ex.state()
        pyr.build(img)
        rc, _, _ = ex.extract_from_pyramid_raw(pyr, 4096)
        assert rc == ERR_INVALID_ARGUMENT and ex.state() == before
        pyr.build_undistorted(u, img)    # the identity: the kept image is the frame
        assert np.array_equal(ex.extract_from_pyramid(pyr), _first_list(kind, img))
        pyr.build(img)                   # a plain build drops the kept image again
        rc, _, _ = ex.extract_from_pyramid_raw(pyr, 4096)
        assert rc == ERR_INVALID_ARGUMENT
    finally:
        ex.close()
        pyr.close()
        u.close()

