"""dsopp_hip_undistorter_create_from_model (camera_remap.hip) against the NumPy model of tests/camera_remap_model.py.
Simple-radial maps are held bit for bit (products, sums and square roots only).  TUM-FOV and atan maps go through the device's atan2:
an entry may differ by one float32 ulp, only where the model's binary64 value lies within 64 of its spacings of a float32 rounding
midpoint (the device atan2's documented accuracy followed by five roundings), and at most 1e-4 of a case's entries may be left out so;
the model alone leaves out none at these sizes.  Success flags are equal except where the model's point lies within 1e-9 px of a ROI
bound.  The table is held through its only reader: an undistorter built from the model and one built by dsopp_hip_undistorter_create
from the device's own maps produce the same bytes.  The sizes cover every width mod 4, more than one workgroup, rows that end inside a
thread's four pixels, and the two sizes with one and no successful entry."""
import ctypes as C
import functools

import numpy as np
import pytest

import camera_remap_model as cm

pytestmark = pytest.mark.gpu

SIZES = [(160, 120), (163, 121), (64, 48), (31, 17), (259, 67), (9, 9), (8, 8)]
CASES = [(size, name) for size in SIZES for name in cm.CAMERAS]
PRODUCTION = ((1280, 1024), "fov")
MIDPOINT_SPACINGS, LEFT_OUT_SHARE, ROI_GUARD = 64.0, 1e-4, 1e-9
ERR_INVALID_ARGUMENT = -1


_OPEN = []


@pytest.fixture(scope="module", autouse=True)
def _close_cached_undistorters():
    yield
    for u in _OPEN:
        u.close()
    _OPEN.clear()
    _device.cache_clear()


def _id(case):
    return f"{case[0][0]}x{case[0][1]}-{case[1]}"


def _model(size, name):
    from dsopp_amd import capi
    camera = cm.CAMERAS[name](*size)
    if camera[0] == cm.SIMPLE_RADIAL:
        return capi.CameraModel.simple_radial(size, *camera[1:])
    if camera[0] == cm.TUM_FOV:
        return capi.CameraModel.tum_fov(size, *camera[1:])
    return capi.CameraModel.atan(size, *camera[1:5], camera[5:])


@functools.lru_cache(maxsize=None)
def _device(size, name):
    """the undistorter built from the model, with its maps read back; kept for the whole module"""
    from dsopp_amd import capi
    u = capi.Undistorter.from_model(_model(size, name), maps=True)
    _OPEN.append(u)
    u.map_x.setflags(write=False)
    u.map_y.setflags(write=False)
    return u


@functools.lru_cache(maxsize=None)
def _expected(size, name):
    """the model's tables; a simple-radial model is fed the library's own max_valid_radius"""
    from dsopp_amd import capi
    camera = cm.CAMERAS[name](*size)
    radius = capi.camera_model_to_pinhole(_model(size, name))[1][0] if camera[0] == cm.SIMPLE_RADIAL else None
    return cm.tables(size[0], size[1], camera, radius)


@functools.lru_cache(maxsize=None)
def _images(size):
    w, h = size
    random = np.random.default_rng(w * 131 + h).integers(0, 256, (h, w)).astype(np.uint8)
    horizontal = np.broadcast_to((np.arange(w) * 255 // max(w - 1, 1)).astype(np.uint8), (h, w)).copy()
    vertical = np.broadcast_to((np.arange(h) * 255 // max(h - 1, 1)).astype(np.uint8)[:, None], (h, w)).copy()
    return random, horizontal, vertical


def _check_maps(size, name):
    w, h = size
    u, t = _device(size, name), _expected(size, name)
    assert np.array_equal(u.pinhole_intrinsics, cm.pinhole_intrinsics(w, h, cm.CAMERAS[name](w, h)))
    got_ok = u.map_x != -1
    assert np.array_equal(got_ok, u.map_y != -1)
    if name.startswith("sr_"):
        assert np.array_equal(got_ok, t.ok), (size, name, int((got_ok != t.ok).sum()))
        assert np.array_equal(u.map_x, t.map_x) and np.array_equal(u.map_y, t.map_y), (size, name)
        return
    # the model alone: no entry near a rounding midpoint beyond the stated share, no point on a ROI bound
    near = ((cm.spacings_to_midpoint(t.px) <= MIDPOINT_SPACINGS) | (cm.spacings_to_midpoint(t.py) <= MIDPOINT_SPACINGS)) & t.ok
    assert near.mean() <= 3.3e-6 and (near.sum() == 0 or size == PRODUCTION[0]), (size, name, int(near.sum()))
    on_bound = t.in_border & (cm.spacings_to_roi_bound(t, w, h) <= ROI_GUARD)
    assert not on_bound.any(), (size, name, int(on_bound.sum()))
    assert np.array_equal(got_ok[~on_bound], t.ok[~on_bound]), (size, name, int((got_ok != t.ok).sum()))
    both = got_ok & t.ok
    left_out = np.zeros_like(both)
    worst = 0.0
    for got, want, exact in ((u.map_x, t.map_x, t.px), (u.map_y, t.map_y, t.py)):
        differs = both & (got != want)
        if differs.any():
            distance = cm.spacings_to_midpoint(exact[differs])
            worst = max(worst, float(distance.max()))
            assert np.array_equal(np.nextafter(want[differs], got[differs]), got[differs]), (size, name, "more than one ulp")
            assert (distance <= MIDPOINT_SPACINGS).all(), (size, name, float(distance.max()))
        left_out |= differs
    print(f"camera_remap {_id((size, name))}: {int(left_out.sum())} of {left_out.size} entries one ulp off, "
          f"greatest distance from a midpoint {worst:.2f} spacings")
    assert left_out.mean() <= LEFT_OUT_SHARE, (size, name, int(left_out.sum()))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_maps_match_the_model(case):
    _check_maps(*case)


def _check_table(size, name):
    """the folded table through the remap: against an undistorter created from the device's own maps"""
    import torch
    from dsopp_amd import capi
    w, h = size
    u = _device(size, name)
    assert u.sizes() == (size, size)
    v = capi.Undistorter(size, size, u.map_x, u.map_y)
    try:
        for image in _images(size):
            first, second = u.undistort(image), v.undistort(image)
            assert np.array_equal(first, second), (size, name, int((first != second).sum()))
        bgr = np.random.default_rng(w + 7 * h).integers(0, 256, (h, w, 3)).astype(np.uint8)
        d_in = torch.from_numpy(bgr).cuda()
        outs = []
        for handle in (u, v):
            d_bgr = torch.zeros(3 * w * h + 8, dtype=torch.uint8, device="cuda")
            d_grey = torch.zeros(w * h + 8, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            handle.undistort_bgr_device(d_in.data_ptr(), d_bgr.data_ptr(), d_grey.data_ptr())
            torch.cuda.synchronize()
            outs.append((d_bgr.cpu().numpy(), d_grey.cpu().numpy()))
        assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]), (size, name)
    finally:
        v.close()


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_table_equals_the_fold_of_the_maps(case):
    _check_table(*case)


def test_production_size():
    """1280 x 1024: table offsets beyond 2^16 and thousands of workgroups"""
    _check_maps(*PRODUCTION)
    _check_table(*PRODUCTION)


@pytest.mark.parametrize("name", ["sr_mild", "fov", "atan_poly"])
def test_pyramid_build_undistorted(name):
    from dsopp_amd import capi
    size = (64, 48)
    u = _device(size, name)
    v = capi.Undistorter(size, size, u.map_x, u.map_y)
    a, b = capi.Pyramid(64, 48, 3), capi.Pyramid(64, 48, 3)
    try:
        image = _images(size)[0]
        a.build_undistorted(u, image)
        b.build_undistorted(v, image)
        for level in range(3):
            assert np.array_equal(a.get_level(level), b.get_level(level)), (name, level)
        assert np.abs(a.get_level(2)[..., 1:]).max() > 0
    finally:
        a.close()
        b.close()
        v.close()


def _raw_create(model, map_x, map_y, pinhole=None, want_handle=True):
    from dsopp_amd import capi
    h = C.c_void_p()
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = capi.lib().dsopp_hip_undistorter_create_from_model(0, None, None if model is None else C.byref(model), ptr(map_x), ptr(map_y), ptr(pinhole),
                                                            C.byref(h) if want_handle else None)
    return rc, h


@pytest.mark.parametrize("size", [(163, 121), (31, 17), (64, 48)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_guard_floats_round_both_maps_stay(size):
    from dsopp_amd import capi
    n, guard = size[0] * size[1], 16
    want = _device(size, "fov")
    bufs = [np.full(n + 2 * guard, np.float32(-77.25)) for _ in range(2)]
    rc, h = _raw_create(_model(size, "fov"), bufs[0][guard:], bufs[1][guard:])
    assert rc == 0 and h.value
    capi.lib().dsopp_hip_undistorter_destroy(h)
    for buf, m in zip(bufs, (want.map_x, want.map_y)):
        assert (buf[:guard] == np.float32(-77.25)).all() and (buf[guard + n:] == np.float32(-77.25)).all()
        assert np.array_equal(buf[guard:guard + n].reshape(m.shape), m)


@pytest.mark.parametrize("case", [((163, 121), "sr_leaves_roi"), ((31, 17), "fov_off_centre"), ((259, 67), "atan_poly")], ids=_id)
def test_without_map_outputs(case):
    from dsopp_amd import capi
    size, name = case
    u = capi.Undistorter.from_model(_model(size, name))
    try:
        assert u.map_x is None and u.map_y is None
        assert np.array_equal(u.pinhole_intrinsics, _device(size, name).pinhole_intrinsics)
        for image in _images(size):
            assert np.array_equal(u.undistort(image), _device(size, name).undistort(image))
    finally:
        u.close()


def test_repeated_and_interleaved_calls_give_identical_bytes():
    from dsopp_amd import capi
    a_case, b_case = ((163, 121), "fov"), ((259, 67), "atan_poly")
    made = []
    try:
        for case in (a_case, b_case, a_case, b_case, b_case, a_case):
            made.append((case, capi.Undistorter.from_model(_model(*case), maps=True)))
        for case, u in made:
            first = _device(*case)
            assert np.array_equal(u.map_x, first.map_x) and np.array_equal(u.map_y, first.map_y)
        for image_index in range(3):   # interleaved use of every handle
            outs = [(case, u.undistort(_images(case[0])[image_index])) for case, u in made]
            for case, out in outs:
                assert np.array_equal(out, _device(*case).undistort(_images(case[0])[image_index]))
    finally:
        for _, u in made:
            u.close()


def test_refusals_then_a_good_create_works():
    size = (64, 48)
    n = size[0] * size[1]
    mx, my = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    good = lambda: _model(size, "sr_mild")
    fov = lambda: _model(size, "fov")
    atan = lambda: _model(size, "atan_plain")

    def changed(make, **kw):
        m = make()
        for field, v in kw.items():
            if isinstance(v, tuple):
                getattr(m, field)[v[0]] = v[1]
            else:
                setattr(m, field, v)
        return m

    def refused(model, map_x=None, map_y=None, want_handle=True):
        rc, h = _raw_create(model, map_x, map_y, want_handle=want_handle)
        assert not h.value
        return rc == ERR_INVALID_ARGUMENT

    assert refused(None) and refused(good(), want_handle=False)
    assert refused(good(), mx, None) and refused(good(), None, my)
    assert refused(changed(good, type=3)) and refused(changed(good, type=-1))
    for bad in (np.nan, np.inf):
        assert refused(changed(good, params=(0, bad))) and refused(changed(good, params=(2, bad))) and refused(changed(good, k=(0, bad)))
        assert refused(changed(fov, params=(1, bad))) and refused(changed(fov, k=(0, bad)))
        assert refused(changed(atan, num_k=2, k=(1, bad)))
    assert refused(changed(good, params=(0, 0.0))) and refused(changed(good, params=(0, -3.0)))
    assert refused(changed(fov, params=(0, 0.0))) and refused(changed(fov, params=(1, -1.0))) and refused(changed(atan, params=(1, 0.0)))
    for bad in (0.0, -0.5, np.pi, 3.5):
        assert refused(changed(fov, k=(0, bad)))
    assert refused(changed(good, num_k=1)) and refused(changed(good, num_k=3)) and refused(changed(fov, num_k=0)) and refused(changed(fov, num_k=2))
    assert refused(changed(atan, num_k=17)) and refused(changed(atan, num_k=-1))
    assert refused(changed(good, width=1)) and refused(changed(good, height=1)) and refused(changed(good, width=0))
    assert refused(changed(good, width=65536, height=32768))
    pinhole = np.zeros(4)
    rc, h = _raw_create(good(), mx, my, pinhole)
    assert rc == 0 and h.value
    from dsopp_amd import capi
    capi.lib().dsopp_hip_undistorter_destroy(h)
    assert np.array_equal(mx.reshape(48, 64), _device(size, "sr_mild").map_x) and pinhole.tolist() == [0.8 * 64, 0.8 * 64, 32.0, 24.0]


# ---- the set-up driver over the C-ABI alone against the same calls through the binding

def _hex_image(name, image):
    h, w = image.shape
    return [f"{name} {w} {h}"] + ["".join(f"{v:02x}" for v in row) for row in image.tolist()]


def _bits(values):
    return " ".join(f"{v:016x}" for v in np.asarray(values, dtype=np.float64).view(np.uint64).tolist())


def test_driver_equals_the_binding(tmp_path):
    """dsopp_amd/host/example_camera_setup.cpp on its built-in TUM-FOV calibration: calibration, transformed calibration, mask, vignette"""
    import subprocess
    from dsopp_amd import capi
    from test_camera_remap import build_example
    r = subprocess.run([build_example(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    w, h, ratio, crop = 160, 120, 0.75, 3
    params = [0.7 * w, 0.72 * h, 0.51 * w, 0.48 * h]
    u = capi.Undistorter.from_model(capi.CameraModel.tum_fov((w, h), *params, 0.93))
    t = capi.Transformer((w, h), ratio, crop)
    try:
        x, y = np.meshgrid(np.arange(w), np.arange(h))
        mask = np.where((y >= h - h // 6) | ((x >= w // 3) & (x < w // 3 + 9) & (y >= 10) & (y < 21)), 0, 255).astype(np.uint8)
        dx, dy = 2 * x - w, 2 * y - h
        vignette = (255 - (dx * dx + dy * dy) * 150 // (w * w + h * h)).astype(np.uint8)
        image_size, intrinsics, _ = capi.transform_calibration((w, h), ratio, crop, u.pinhole_intrinsics)
        want = ["calibration pinhole " + _bits([w, h] + u.pinhole_intrinsics.tolist()), f"model 1 {w} {h} 1 " + _bits(params + [0.93]),
                "transformed " + _bits(image_size.tolist() + intrinsics.tolist())]
        want += _hex_image("mask", t.transform_mask(u.undistort(mask))) + _hex_image("vignette", t.transform_image(u.undistort(vignette)))
        got = r.stdout.splitlines()
        assert len(got) == len(want) and got == want, [(i, a, b) for i, (a, b) in enumerate(zip(got, want)) if a != b][:3]
        assert len(set(got[4:4 + t.out_size[1]])) > 3    # the mask has structure
    finally:
        t.close()
        u.close()
