"""tests/camera_remap_model.py, the NumPy statement of the remap tables built from a camera model (include/dsopp_hip.h,
dsopp_hip_undistorter_create_from_model), pinned on hand cases, against the older helpers of tests/undistort_model.py, through its own
inverse and on the reference's "three points on a line" test; and dsopp_hip_camera_model_to_pinhole — which needs no device — against
numpy.roots.  tests/test_gpu_camera_remap.py holds the device to the model."""
import ctypes as C

import numpy as np
import pytest

import camera_remap_model as cm
import undistort_model as um

SIZES = [(160, 120), (163, 121)]


# ---- hand cases: no distortion, a power-of-two focal length and the centre at size / 2 make every step exact

@pytest.mark.parametrize("size", [(32, 24), (33, 19), (160, 120)])
def test_zero_distortion_is_the_identity_inside_the_border(size):
    w, h = size
    t = cm.Tables(w, h, (cm.SIMPLE_RADIAL, 64.0, w / 2.0, h / 2.0, 0.0, 0.0))
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    inside = (x >= 4) & (x <= w - 5) & (y >= 4) & (y <= h - 5)
    assert np.array_equal(t.ok, inside)
    assert np.array_equal(t.map_x[inside], x[inside].astype(np.float32)) and np.array_equal(t.map_y[inside], y[inside].astype(np.float32))
    assert (t.map_x[~inside] == -1).all() and (t.map_y[~inside] == -1).all()


def test_8x8_has_no_entry_and_9x9_has_one():
    t = cm.Tables(8, 8, (cm.SIMPLE_RADIAL, 8.0, 4.0, 4.0, 0.0, 0.0))
    assert not t.ok.any() and (t.map_x == -1).all() and (t.map_y == -1).all()
    t = cm.Tables(9, 9, (cm.SIMPLE_RADIAL, 8.0, 4.5, 4.5, 0.0, 0.0))
    assert t.ok.sum() == 1 and t.ok[4, 4] and (t.map_x[4, 4], t.map_y[4, 4]) == (4.0, 4.0)
    assert (t.map_x[~t.ok] == -1).all()


# ---- against the helpers the undistorter's tests have used so far (they divide where the reference multiplies by the inverse)

def _ulps(a, b):
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32))


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", ["sr_mild", "sr_leaves_roi", "sr_radius", "fov", "fov_off_centre"])
def test_agrees_with_the_older_helpers_within_one_ulp(name, size):
    w, h = size
    camera = cm.CAMERAS[name](w, h)
    t = cm.tables(w, h, camera)
    old_x, old_y = (um.simple_radial_maps if camera[0] == cm.SIMPLE_RADIAL else um.tum_fov_maps)(w, h, *camera[1:])
    assert np.array_equal(old_x == -1, ~t.ok)
    assert _ulps(t.map_x, old_x).max() <= 1 and _ulps(t.map_y, old_y).max() <= 1


# ---- the GPU tests' cameras reach the branches they are meant to reach

@pytest.mark.parametrize("size", SIZES + [(64, 48), (31, 17), (259, 67)])
def test_failure_branches_cover_a_share_of_the_pixels(size):
    w, h = size
    share = lambda name, reason: (cm.tables(w, h, cm.CAMERAS[name](w, h)).reason == reason).mean()
    assert share("sr_leaves_roi", cm.ROI) >= 0.01
    assert share("sr_radius", cm.RADIUS) >= 0.01
    assert share("fov_off_centre", cm.ROI) >= 0.01
    for name in cm.CAMERAS:
        t = cm.tables(w, h, cm.CAMERAS[name](w, h))
        assert (~t.in_border).mean() >= 0.10 and t.ok.mean() >= 0.2, name


# ---- every successful entry goes back to its pinhole ray

@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", cm.CAMERAS)
def test_inverse_gives_the_pinhole_ray(name, size):
    w, h = size
    camera = cm.CAMERAS[name](w, h)
    t = cm.tables(w, h, camera)
    assert t.ok.sum() > 0.2 * w * h
    r_max = np.hypot(t.rx, t.ry)[t.ok].max() * (1 + 1e-12)
    rx, ry = cm.unproject(camera, t.px[t.ok], t.py[t.ok], r_max)
    assert np.abs(rx - t.rx[t.ok]).max() <= 1e-9 and np.abs(ry - t.ry[t.ok]).max() <= 1e-9


# ---- the reference's own data-free test (test/test/sensors/camera/calibration/undistorter.cpp:91-138), 10 lines of 3 points

@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", ["sr_mild", "fov"])
def test_three_points_on_a_line(name, size):
    w, h = size
    camera = cm.CAMERAS[name](w, h)
    t = cm.tables(w, h, camera)
    fx, fy, cx, cy = cm.pinhole_intrinsics(w, h, camera)
    rng = np.random.default_rng(w + len(name))
    checked = 0
    for _ in range(10):
        k, b = rng.uniform(-0.6, 0.0), rng.uniform(0.5 * h, 0.8 * h)   # y = k x + b
        xs = []
        while len(xs) < 3:
            x = rng.uniform(8, w - 8)
            if all(abs(x - o) >= 5 for o in xs) and 8 <= k * x + b < h - 8:
                xs.append(x)
        xs = np.array(xs)
        ys = k * xs + b
        # the rays of the three pinhole points and their distorted projections
        px, py, ok, _ = cm.project(w, h, camera, (xs - cx) * (1.0 / fx), (ys - cy) * (1.0 / fy))
        assert ok.all()
        img = cm.draw_discs(w, h, [(int(u), int(v)) for u, v in zip(px, py)])
        out = um.remap(img, t.map_x, t.map_y)
        for x, y in zip(xs, ys):
            assert out[int(y), int(x)] > 100, (name, size, x, y)
            checked += 1
    assert checked == 30


# ---- dsopp_hip_camera_model_to_pinhole: the library's own root finder against numpy.roots

def _model(w, h, camera):
    from dsopp_amd import capi
    if camera[0] == cm.SIMPLE_RADIAL:
        return capi.CameraModel.simple_radial((w, h), *camera[1:])
    if camera[0] == cm.TUM_FOV:
        return capi.CameraModel.tum_fov((w, h), *camera[1:])
    return capi.CameraModel.atan((w, h), *camera[1:5], camera[5:])


def _close(got, want, rel):
    if not np.isfinite(want):
        return (np.isnan(want) and np.isnan(got)) or got == want
    return abs(got - want) <= rel * abs(want)


ROOT_CASES = {   # (w, h, f, cx, cy, k1, k2) -> (the least positive root is finite, the extremum rule replaces it)
    "sr_mild": ((160, 120, 128.0, 78.4, 61.2, -0.25, 0.06), True, False),
    "sr_leaves_roi": ((163, 121, 0.8 * 163, 0.49 * 163, 0.51 * 121, 0.4, 0.05), True, False),
    "sr_radius": ((160, 120, 80.0, 80.0, 60.0, -0.6, 0.05), True, True),
    "sr_radius_odd": ((259, 67, 129.5, 129.5, 33.5, -0.6, 0.05), True, True),
    "zero": ((64, 48, 32.0, 32.0, 24.0, 0.0, 0.0), True, False),
    "no_root_then_extremum": ((160, 120, 80.0, 80.0, 60.0, -0.2, -0.05), False, True),
    "no_root_k2_zero": ((160, 120, 80.0, 80.0, 60.0, -0.6, 0.0), False, False),
    "k2_zero_negative_k1": ((160, 120, 128.0, 78.4, 61.2, -0.1, 0.0), True, False),
    "k2_zero_positive_k1": ((160, 120, 128.0, 78.4, 61.2, 0.3, 0.0), True, False),
    "k2_dropped": ((160, 120, 128.0, 78.4, 61.2, -0.1, 1e-10), True, False),
    "cubic_and_quintic_positive": ((31, 17, 24.8, 15.2, 8.7, 0.2, 0.3), True, False),
}


@pytest.mark.parametrize("case", ROOT_CASES)
def test_camera_model_to_pinhole_against_numpy_roots(case):
    from dsopp_amd import capi
    (w, h, f, cx, cy, k1, k2), finite, replaced = ROOT_CASES[case]
    root = cm.minimal_positive_root([-(np.hypot(max(cx, w - cx), max(cy, h - cy)) / f), 1.0, 0.0, k1, 0.0, k2])
    want, was_replaced = cm.simple_radial_derived(w, h, f, cx, cy, k1, k2)
    assert np.isfinite(root) == finite and was_replaced == replaced, (root, want, was_replaced)
    pinhole, derived = capi.camera_model_to_pinhole(capi.CameraModel.simple_radial((w, h), f, cx, cy, k1, k2))
    assert pinhole.tolist() == [f, f, w / 2.0, h / 2.0]
    assert _close(derived[0], want[0], 1e-12), (derived, want)
    assert _close(derived[1], want[1], 1e-10) and _close(derived[2], want[2], 1e-10), (derived, want)


def test_k2_dropped_case_takes_the_cubic_root():
    """1e-10 is below 1e-8 of the normalised polynomial: the root is the cubic's, not the quintic's (they differ in the 10th digit)"""
    w, h, f, cx, cy, k1, k2 = ROOT_CASES["k2_dropped"][0]
    R = np.hypot(max(cx, w - cx), max(cy, h - cy)) / f
    cubic = cm.minimal_positive_root([-R, 1.0, 0.0, k1])
    assert cm.minimal_positive_root([-R, 1.0, 0.0, k1, 0.0, k2]) == cubic


@pytest.mark.parametrize("size", SIZES + [(64, 48), (31, 17), (259, 67), (9, 9), (8, 8)])
@pytest.mark.parametrize("name", cm.CAMERAS)
def test_camera_model_to_pinhole_on_the_test_cameras(name, size):
    from dsopp_amd import capi
    w, h = size
    camera = cm.CAMERAS[name](w, h)
    pinhole, derived = capi.camera_model_to_pinhole(_model(w, h, camera))
    assert np.array_equal(pinhole, cm.pinhole_intrinsics(w, h, camera))
    if camera[0] == cm.SIMPLE_RADIAL:
        want, _ = cm.simple_radial_derived(w, h, *camera[1:])
        assert _close(derived[0], want[0], 1e-12), (derived, want)
    else:
        assert derived.tolist() == [0.0, 0.0, 0.0]


def test_camera_model_to_pinhole_refusals():
    from dsopp_amd import capi
    good = lambda: capi.CameraModel.simple_radial((160, 120), 128.0, 78.4, 61.2, -0.25, 0.06)
    fov = lambda: capi.CameraModel.tum_fov((160, 120), 112.0, 86.4, 81.6, 57.6, 0.93)

    def rc(model):
        out = np.zeros(4)
        return capi.lib().dsopp_hip_camera_model_to_pinhole(None if model is None else C.byref(model), capi._p(out), None)

    def changed(make, **kw):
        m = make()
        for name, v in kw.items():
            if isinstance(v, tuple):
                getattr(m, name)[v[0]] = v[1]
            else:
                setattr(m, name, v)
        return m

    assert rc(good()) == 0 and rc(fov()) == 0
    assert rc(None) == -1
    assert rc(changed(good, type=3)) == -1 and rc(changed(good, type=-1)) == -1
    for bad in (np.nan, np.inf, -np.inf):
        assert rc(changed(good, params=(1, bad))) == -1 and rc(changed(good, k=(1, bad))) == -1 and rc(changed(fov, params=(3, bad))) == -1
    assert rc(changed(good, params=(0, 0.0))) == -1 and rc(changed(good, params=(0, -1.0))) == -1
    assert rc(changed(fov, params=(1, 0.0))) == -1
    for bad in (0.0, -0.1, np.pi, 4.0):
        assert rc(changed(fov, k=(0, bad))) == -1
    assert rc(changed(fov, k=(0, np.nextafter(np.pi, 0.0)))) == 0
    assert rc(changed(good, num_k=1)) == -1 and rc(changed(good, num_k=3)) == -1 and rc(changed(fov, num_k=2)) == -1
    atan = capi.CameraModel.atan((160, 120), 44.8, 44.8, 75.2, 58.8, ())
    assert rc(atan) == 0 and rc(changed(lambda: atan, num_k=16)) == 0
    assert rc(changed(lambda: atan, num_k=17)) == -1 and rc(changed(lambda: atan, num_k=-1)) == -1
    assert rc(changed(good, width=1)) == -1 and rc(changed(good, height=1)) == -1
    assert rc(changed(good, width=65536, height=32768)) == -1     # 2^31 pixels
    assert rc(changed(good, width=65535, height=32768)) == 0


# ---- HipCameraCalibration::parse and the set-up driver (dsopp_amd/host/example_camera_setup.cpp)

def build_example(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "dsopp_amd", "lib")
    exe = str(tmp_path / "example_camera_setup")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", os.path.join(root, "dsopp_amd", "host", "example_camera_setup.cpp"),
                           f"-L{libdir}", "-ldsopp_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", exe])
    return exe


def _bits(values):
    return " ".join(f"{v:016x}" for v in np.asarray(values, dtype=np.float64).view(np.uint64).tolist())


def test_parser_reads_the_three_formats_and_refuses_the_rest(tmp_path):
    import subprocess
    exe = build_example(tmp_path)

    def parse(text, flag="--parse"):
        path = tmp_path / "calib.txt"
        path.write_text(text)
        r = subprocess.run([exe, flag, str(path)], capture_output=True, text=True)
        return r.returncode, r.stdout.splitlines()

    # pinhole (fabric.cpp:23-31): the intrinsics as they stand, no undistorter
    rc, out = parse("pinhole\n640 480\n448.5 460.25 322.5 241.75\n")
    assert rc == 0 and out == ["calibration pinhole " + _bits([640, 480, 448.5, 460.25, 322.5, 241.75]), "model none"]
    # simple_radial with transform_to_pinhole (:33-51): the pinhole of constructRemaps (f, f, w / 2, h / 2) and the model
    rc, out = parse("simple_radial\n163 121\n130.4 79.87 61.71\n-0.25 0.06\n")
    assert rc == 0 and out == ["calibration pinhole " + _bits([163, 121, 130.4, 130.4, 81.5, 60.5]),
                               "model 0 163 121 2 " + _bits([130.4, 79.87, 61.71, 0.0, -0.25, 0.06])]
    # ... and without it (:41-44): the simple-radial calibration itself, Undistorter::Identity
    rc, out = parse("simple_radial\n163 121\n130.4 79.87 61.71\n-0.25 0.06\n", "--parse-native")
    assert rc == 0 and out == ["calibration simple_radial " + _bits([163, 121, 130.4, 79.87, 61.71, -0.25, 0.06]), "model none"]
    rc, out = parse("tum_fov\n640 480\n0.5 0.6 0.5 0.5 0.9\n", "--parse-native")   # :101-104
    assert rc == 1 and out[0].startswith("refused (-1): ")
    # tum_fov (:53-72): focals and centre are relative to the image size
    rc, out = parse("tum_fov\n1280 1024\n0.535719308086809 0.669566858850269 0.493248545285398 0.500408664348414 0.897966326944875\n")
    fx, fy = 0.535719308086809 * 1280.0, 0.669566858850269 * 1024.0
    cx, cy = 0.493248545285398 * 1280.0, 0.500408664348414 * 1024.0
    assert rc == 0 and out == ["calibration pinhole " + _bits([1280, 1024, fx, fy, 640.0, 512.0]),
                               "model 1 1280 1024 1 " + _bits([fx, fy, cx, cy, 0.897966326944875])]
    # the refusals: an unknown type, a text that ends early, a model the library refuses
    for text in ("kannala_brandt\n640 480\n1 1 1 1\n", "", "tum_fov\n640 480\n0.5 0.6 0.5\n", "simple_radial\n640 480\n300 x 240 0 0\n",
                 "tum_fov\n640 480\n0.5 0.6 0.5 0.5 3.5\n", "simple_radial\n640 480\n-300 320 240 0 0\n", "tum_fov\n1 480\n0.5 0.6 0.5 0.5 0.9\n"):
        rc, out = parse(text)
        assert rc == 1 and len(out) == 1 and out[0].startswith("refused (-1): "), (text, rc, out)
    r = subprocess.run([exe, "--parse", str(tmp_path / "missing.txt")], capture_output=True, text=True)
    assert r.returncode == 1 and "could not open" in r.stdout


def test_example_driver_runs_or_fails_loudly_without_gpu(tmp_path):
    import subprocess
    from dsopp_amd import capi
    r = subprocess.run([build_example(tmp_path)], capture_output=True, text=True)
    assert r.stdout.splitlines()[0].startswith("calibration pinhole ")   # the parser ran: it needs no device
    if capi.device_count() > 0:
        assert r.returncode == 0 and "vignette" in r.stdout
    else:
        assert r.returncode == 2 and "no CPU fallback" in r.stdout
