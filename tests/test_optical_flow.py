"""tests/optical_flow_model.py, the NumPy statement of the device optical-flow tracker (include/dsopp_hip.h, dsopp_hip_flow_tracker_create),
pinned on the CPU: pyrDown, the Scharr planes, the level count, the bilinear weights and the tracker itself on an analytic texture whose
shift is known.  tests/test_gpu_optical_flow.py holds the device to the model bit for bit."""
import functools
import os
import subprocess

import numpy as np
import pytest

import optical_flow_model as ofm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIFTS = [(2.3, -1.7), (7.25, 5.5), (-11.5, 3.0)]
SIZES = [(160, 120), (161, 123)]


def texture(width, height, shift=(0.0, 0.0)):
    """a sum of low-frequency sinusoids (wavelengths of 27 to 126 pixels) sampled at (x - shift) and quantised to 8 bits: the content at
    (x, y) of texture(w, h) is at (x + sx, y + sy) of texture(w, h, (sx, sy))"""
    y, x = np.mgrid[0:height, 0:width].astype(np.float64)
    x, y = x - shift[0], y - shift[1]
    v = (128.0 + 34.0 * np.sin(0.110 * x + 0.070 * y) + 30.0 * np.sin(0.050 * x - 0.130 * y + 1.0) +
         26.0 * np.sin(0.170 * x + 0.150 * y + 2.0) + 22.0 * np.cos(0.230 * x - 0.040 * y + 0.5) + 12.0 * np.sin(0.031 * x + 0.220 * y))
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def grid_points(width, height, n=64, margin=28, seed=7):
    """n points at least `margin` pixels from every border, on quarter pixels (so that pt * 2^-level is exact on every level)"""
    rng = np.random.default_rng(seed)
    x = rng.integers(4 * margin, 4 * (width - margin) + 1, n) / 4.0
    y = rng.integers(4 * margin, 4 * (height - margin) + 1, n) / 4.0
    return np.stack([x, y], axis=1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def texture_case(width, height, shift):
    """(reference image, target image, points, the model's (points_to, status, err, iterations)), computed once per session"""
    ref, tgt, pts = texture(width, height), texture(width, height, shift), grid_points(width, height)
    m = ofm.Tracker(width, height)
    m.set_reference(ref)
    return ref, tgt, pts, m.track(tgt, pts)


def test_pyr_down_keeps_a_constant_image():
    for shape in [(17, 31), (48, 64), (9, 7)]:
        assert np.array_equal(ofm.pyr_down(np.full(shape, 93, np.uint8)), np.full(((shape[0] + 1) // 2, (shape[1] + 1) // 2), 93, np.uint8))


def test_pyr_down_of_an_impulse_is_the_5x5_kernel():
    img = np.zeros((21, 23), np.uint8)
    img[10, 12] = 255                                    # even coordinates: the centre tap of output (6, 5)
    k = np.outer([1, 4, 6, 4, 1], [1, 4, 6, 4, 1])
    out = ofm.pyr_down(img).astype(np.int64)
    # the output pixel at (5 + j, 6 + i) reads the impulse with taps (2 - 2 j, 2 - 2 i): only the even taps 1, 6, 1 land on it
    expect = np.zeros_like(out)
    for j in (-1, 0, 1):
        for i in (-1, 0, 1):
            expect[5 + j, 6 + i] = (k[2 - 2 * j, 2 - 2 * i] * 255 + 128) >> 8
    assert np.array_equal(out, expect) and expect[5, 6] == (36 * 255 + 128) >> 8
    img = np.zeros((21, 23), np.uint8)
    img[11, 13] = 255                                    # odd coordinates: the 4-taps of the four neighbours
    out = ofm.pyr_down(img).astype(np.int64)
    expect = np.zeros_like(out)
    expect[5:7, 6:8] = (16 * 255 + 128) >> 8
    assert np.array_equal(out, expect)
    # and the full 5 x 5 weights, read off by moving the impulse under one output pixel
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            img = np.zeros((21, 23), np.uint8)
            img[10 + dy, 12 + dx] = 255
            assert ofm.pyr_down(img)[5, 6] == (k[dy + 2, dx + 2] * 255 + 128) >> 8


def test_pyr_down_odd_size_edge_by_hand():
    """5 x 5 -> 3 x 3: the last output column is centred on source column 4 and reads columns 2 3 4 3 2 (REFLECT_101), as the rows do"""
    img = (np.arange(5)[None, :] * 10 + np.arange(5)[:, None] * 50).astype(np.uint8)    # 10 x + 50 y
    out = ofm.pyr_down(img)
    assert out.shape == (3, 3)
    # a separable image: horizontal sums of x -> 16 * (1.25, 2, 2.75) * 10 by the reflected taps; 1*2+4*1+6*0+4*1+1*2 = 12, 32, 2+12+24+12+2 = 52
    hx = np.array([12, 32, 52]) * 10                     # sum of taps * 10 x at output columns 0, 1, 2
    hy = np.array([12, 32, 52]) * 50
    expect = (16 * hx[None, :] + 16 * hy[:, None] + 128) >> 8
    assert np.array_equal(out, expect.astype(np.uint8))
    assert out[2, 2] == (16 * 520 + 16 * 2600 + 128) >> 8 == 195


def test_scharr_of_a_horizontal_ramp():
    s = 3
    img = np.tile((np.arange(20) * s + 7).astype(np.uint8), (11, 1))
    d = ofm.scharr(img)
    assert d.dtype == np.int16 and d.shape == (11, 20, 2)
    assert np.all(d[:, 1:-1, 0] == 32 * s) and np.all(d[..., 1] == 0)
    # the border columns: x - 1 reflects to column 1 at x = 0 and x + 1 to column 18 at x = 19, so both taps read one pixel: dx = 0
    assert np.all(d[:, 0, 0] == 0) and np.all(d[:, -1, 0] == 0)
    # a vertical ramp: dy = 32 s inside, 0 on the reflected border rows, dx = 0
    d = ofm.scharr(img.T.copy())
    assert np.all(d[1:-1, :, 1] == 32 * s) and np.all(d[0, :, 1] == 0) and np.all(d[-1, :, 1] == 0) and np.all(d[..., 0] == 0)
    # extremes stay within int16: a 0 / 255 step gives +-(3 + 10 + 3) * 255
    step = np.zeros((5, 6), np.uint8)
    step[:, 3:] = 255
    assert ofm.scharr(step)[2, 2, 0] == 4080 and ofm.scharr(step)[2, 3, 0] == 4080 and ofm.scharr(255 - step)[2, 2, 0] == -4080


def test_level_counts():
    assert [ofm.num_levels(w, h, 15, 3) for w, h in [(160, 120), (161, 123), (64, 48), (31, 17)]] == [3, 4, 2, 1]
    assert ofm.num_levels(1280, 1024, 15, 3) == 4 and ofm.num_levels(1280, 1024, 15, 0) == 1 and ofm.num_levels(2, 2, 15, 3) == 1
    assert [l.shape for l in ofm.build_levels(np.zeros((123, 161), np.uint8))] == [(123, 161), (62, 81), (31, 41), (16, 21)]


def test_weights_sum_and_ties():
    rng = np.random.default_rng(1)
    for a, b in rng.random((200, 2)).astype(np.float32):
        w = ofm.weights(a, b)
        assert sum(w) == 16384 and min(w) >= -1
    assert ofm.weights(0.0, 0.0) == (16384, 0, 0, 0)
    assert ofm.weights(0.5, 0.5) == (4096, 4096, 4096, 4096)
    # ties round to even: (1 - a)(1 - b) * 16384 = 8191.5 -> 8192, a (1 - b) * 16384 = 0.5 -> 0
    a = np.float32(1.0 / 16384.0)
    assert ofm.weights(a, 0.5) == (8192, 0, 8192, 0)
    a = np.float32(3.0 / 16384.0)                        # 8190.5 -> 8190, 1.5 -> 2
    assert ofm.weights(a, 0.5) == (8190, 2, 8190, 2)


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("shift", SHIFTS)
def test_tracks_a_shifted_texture(size, shift):
    """the model alone stays under 0.35 px on this texture (measured: see the printed figure), so the bound of 0.5 px holds"""
    ref, tgt, pts, (to, status, err, iters) = texture_case(size[0], size[1], shift)
    worst = np.abs(to - pts - np.float32(shift)).max()
    print(f"{size} shift {shift}: worst |result - pt - shift| = {worst:.4f} px, passes per level max {iters.max(axis=0)}, err max {err.max():.3f}")
    assert np.all(status == 1)
    assert worst <= 0.5
    assert worst < 0.35                                  # the texture's own margin: the device test relies on the 0.5 bound


def test_zero_shift_returns_the_point_after_one_pass_per_level():
    ref, pts = texture(161, 123), grid_points(161, 123)
    m = ofm.Tracker(161, 123)
    m.set_reference(ref)
    to, status, err, iters = m.track(ref, pts)
    assert np.array_equal(to, pts) and np.all(status == 1) and np.all(err == 0) and np.all(iters == 1)


def test_flat_image_is_lost_where_it_started():
    flat, pts = np.full((123, 161), 77, np.uint8), grid_points(161, 123)
    m = ofm.Tracker(161, 123)
    m.set_reference(flat)
    to, status, err, iters = m.track(flat, pts)
    assert np.array_equal(to, pts) and np.all(status == 0) and np.all(iters == 0) and np.all(err == 0)


def test_window_origin_at_minus_win_passes_the_range_test_and_one_pixel_further_does_not():
    """pt - half = -win exactly passes the range test (ip.x < -win fires one pixel further).  In the outputs both read status 0: at
    ip.x = -win the window holds one column of the level, column 0, read with the weight of its left neighbour outside the level; the
    derivative planes read 0 there and dx of column 0 is t0[1] - t0[1] = 0 by REFLECT_101, so Ix = 0 over the whole window, A11 = 0,
    D = -A12 * A12 <= 0 and step 4 refuses the point (rows alike: dy of row 0 is 0).  No image makes such a point status 1 under the
    stated arithmetic, so the boundary itself is pinned on the predicate and the outputs on what both routes give."""
    win = 15
    assert not ofm._outside(-win, 5, win, 64, 48) and ofm._outside(-win - 1, 5, win, 64, 48)
    assert not ofm._outside(5, -win, win, 64, 48) and ofm._outside(5, -win - 1, win, 64, 48)
    assert not ofm._outside(63, 47, win, 64, 48) and ofm._outside(64, 47, win, 64, 48) and ofm._outside(63, 48, win, 64, 48)
    for ref in (texture(64, 48), np.random.default_rng(3).integers(0, 256, (48, 64)).astype(np.uint8)):
        m = ofm.Tracker(64, 48, max_level=0)
        m.set_reference(ref)
        pts = np.array([[-8.0, 20.0], [-9.0, 20.0], [20.0, -8.0], [20.0, -9.0], [-7.5, 20.25]], np.float32)    # half = 7: -8 - 7 = -15 = -win
        to, status, err, iters = m.track(ref, pts)
        assert status.tolist() == [0, 0, 0, 0, 0] and np.array_equal(to, pts) and np.all(iters == 0) and np.all(err == 0)
        # the derivative window at ip.x = -win is all zero, the intensity window is not
        w4 = ofm.weights(0.5, 0.25)
        assert not ofm.sample_deriv(m.derivatives[0][..., 0], -win, 13, win, w4).any()
        assert not ofm.sample_deriv(m.derivatives[0][..., 1], 13, -win, win, w4).any()
        assert ofm.sample_image(ref, -win, 13, win, w4, 9).any()


def test_no_cpu_fallback():
    from dsopp_amd import capi
    if capi.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(capi.HipError) as e:
        capi.OpticalFlowTracker(64, 48)
    assert "no HIP device" in str(e.value) or "-4" in str(e.value)


def build_example(tmp_path):
    libdir = os.path.join(ROOT, "dsopp_amd", "lib")
    exe = str(tmp_path / "example_optical_flow")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "dsopp_amd", "host", "example_optical_flow.cpp"),
                           f"-L{libdir}", "-ldsopp_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", exe])
    return exe


def test_example_driver_compiles_and_fails_loudly_without_gpu(tmp_path):
    from dsopp_amd import capi
    exe = build_example(tmp_path)
    if capi.device_count() > 0:
        pytest.skip("GPU present: tests/test_gpu_optical_flow.py runs it")
    r = subprocess.run([exe, "/nonexistent"], capture_output=True, text=True)
    assert r.returncode == 2 and "no CPU fallback" in r.stdout
