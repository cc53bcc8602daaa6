"""The device optical-flow tracker (dsopp_hip_flow_tracker, dsopp_amd/csrc/optical_flow.hip) against tests/optical_flow_model.py: level
images and Scharr planes bit for bit, and status, points, err and the passes per level of every track() exactly — the window sums are
integers and every float step is a single IEEE operation, so there is nothing to tolerate."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import optical_flow_model as ofm
import test_optical_flow as tof

pytestmark = pytest.mark.gpu

PLANE_SIZES = [(160, 120), (161, 123), (64, 48), (31, 17), (2, 2), (259, 67)]


def _image(kind, width, height, seed=0):
    rng = np.random.default_rng(1000 * width + height + seed)
    if kind == "random":
        return rng.integers(0, 256, (height, width)).astype(np.uint8)
    return (rng.integers(0, 2, (height, width)) * 255).astype(np.uint8)      # 0 / 255 extremes


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_planes(tracker, which, levels, derivatives=None):
    assert tracker.num_levels == len(levels)
    for l, want in enumerate(levels):
        if derivatives is None:
            got = tracker.get_level(which, l)
        else:
            got, der = tracker.get_level(which, l, with_derivatives=True)
            assert np.array_equal(der, derivatives[l]), f"Scharr plane of level {l}"
        assert np.array_equal(got, want), f"image of level {l}"


def _assert_track(got, want, what=""):
    to, status, err, iters = got
    wto, wstatus, werr, witers = want
    assert np.array_equal(iters, witers), f"{what}: passes per level differ first at point {np.argwhere(iters != witers)[:1]}"
    assert np.array_equal(status, wstatus), what
    assert np.array_equal(_bits(to), _bits(wto)), f"{what}: points differ at {np.argwhere(_bits(to) != _bits(wto))[:3]}"
    assert np.array_equal(_bits(err), _bits(werr)), what


@pytest.mark.parametrize("kind", ["random", "extremes"])
@pytest.mark.parametrize("size", PLANE_SIZES)
def test_planes_from_a_host_image(size, kind):
    from dsopp_amd import capi
    w, h = size
    ref, tgt = _image(kind, w, h), _image(kind, w, h, seed=1)
    m = ofm.Tracker(w, h)
    m.set_reference(ref)
    t = capi.OpticalFlowTracker(w, h)
    t.set_reference(ref)
    _assert_planes(t, 0, m.reference, m.derivatives)
    t.track(tgt, np.zeros((0, 2), np.float32))                                  # n = 0: the target's levels alone
    _assert_planes(t, 1, ofm.build_levels(tgt))
    _assert_planes(t, 0, m.reference, m.derivatives)                            # the reference is kept
    # a host image with a row stride of its own
    wide = np.zeros((h, w + 7), np.uint8)
    wide[:, :w] = tgt
    t.set_reference(wide[:, :w])
    m.set_reference(tgt)
    _assert_planes(t, 0, m.reference, m.derivatives)
    t.close()


@pytest.mark.parametrize("size", PLANE_SIZES)
def test_planes_from_a_device_pointer_with_a_stride(size):
    """the image in HBM at an odd address with rows 5 bytes longer than the width"""
    import torch
    from dsopp_amd import capi
    w, h = size
    ref, tgt = _image("random", w, h, seed=2), _image("extremes", w, h, seed=3)
    stride = w + 5
    bufs = []
    for img in (ref, tgt):
        host = np.full(h * stride + 1, 0x5A, np.uint8)
        host[1:].reshape(h, stride)[:, :w] = img
        bufs.append(torch.from_numpy(host).cuda())
    torch.cuda.synchronize()
    m = ofm.Tracker(w, h)
    m.set_reference(ref)
    t = capi.OpticalFlowTracker(w, h)
    t.set_reference_device(bufs[0].data_ptr() + 1, stride)
    _assert_planes(t, 0, m.reference, m.derivatives)
    t.track_device(bufs[1].data_ptr() + 1, np.zeros((0, 2), np.float32), stride)
    _assert_planes(t, 1, ofm.build_levels(tgt))
    t.close()


@pytest.mark.parametrize("size", PLANE_SIZES)
def test_planes_from_a_pyramid_after_build_transformed(size):
    """the grey image a pyramid keeps behind build_transformed (a frame of twice the size at ratio 0.5), with no host copy"""
    from dsopp_amd import capi
    w, h = size
    tr = capi.Transformer((2 * w, 2 * h), resize_ratio=0.5, crop_levels=0)
    assert tr.out_size == (w, h)
    p = capi.Pyramid(w, h, 1)
    t = capi.OpticalFlowTracker(w, h)
    for which, seed in ((0, 4), (1, 5)):
        p.build_transformed(None, tr, _image("random", 2 * w, 2 * h, seed=seed))
        kept = p.get_image(1)
        assert kept is not None and kept.shape == (h, w)
        if which == 0:
            t.set_reference(p)
            m = ofm.Tracker(w, h)
            m.set_reference(kept)
            _assert_planes(t, 0, m.reference, m.derivatives)
        else:
            t.track(p, np.zeros((0, 2), np.float32))
            _assert_planes(t, 1, ofm.build_levels(kept))
    t.close()
    p.close()
    tr.close()


@pytest.mark.parametrize("size", tof.SIZES)
@pytest.mark.parametrize("shift", tof.SHIFTS)
def test_tracks_the_shifted_texture_as_the_model_does(size, shift):
    from dsopp_amd import capi
    ref, tgt, pts, want = tof.texture_case(size[0], size[1], shift)
    t = capi.OpticalFlowTracker(*size)
    t.set_reference(ref)
    got = t.track(tgt, pts, with_iterations=True)
    _assert_track(got, want, f"{size} {shift}")
    assert np.all(got[1] == 1) and np.abs(got[0] - pts - np.float32(shift)).max() <= 0.5
    t.close()


@functools.lru_cache(maxsize=None)
def _random_case():
    """two unrelated random-byte images and 80 points in and around them: every pass count, both break branches and status 0 by every route"""
    w, h = 161, 123
    ref, tgt = _image("random", w, h, seed=6), _image("random", w, h, seed=7)
    rng = np.random.default_rng(11)
    pts = np.stack([rng.uniform(-20, w + 20, 80), rng.uniform(-20, h + 20, 80)], axis=1).astype(np.float32)
    m = ofm.Tracker(w, h)
    m.set_reference(ref)
    return ref, tgt, pts, m.track(tgt, pts)


def test_tracks_unrelated_random_images_as_the_model_does():
    from dsopp_amd import capi
    ref, tgt, pts, want = _random_case()
    assert 0 < want[1].sum() < 80 and want[3].max() == 10 and want[3].min() == 0     # the case does exercise the branches
    t = capi.OpticalFlowTracker(161, 123)
    t.set_reference(ref)
    _assert_track(t.track(tgt, pts, with_iterations=True), want, "random images")
    t.close()


def test_flat_image():
    from dsopp_amd import capi
    flat, pts = np.full((123, 161), 77, np.uint8), tof.grid_points(161, 123)
    m = ofm.Tracker(161, 123)
    m.set_reference(flat)
    t = capi.OpticalFlowTracker(161, 123)
    t.set_reference(flat)
    got = t.track(flat, pts, with_iterations=True)
    _assert_track(got, m.track(flat, pts), "flat")
    assert np.all(got[1] == 0) and np.array_equal(got[0], pts)
    t.close()


@functools.lru_cache(maxsize=None)
def _many_points_case():
    """257 points on the shifted texture, some of them outside the image; a track() of the first n is the model's first n rows"""
    w, h, shift = 161, 123, tof.SHIFTS[0]
    rng = np.random.default_rng(5)
    pts = np.stack([rng.uniform(-10, w + 10, 257), rng.uniform(-10, h + 10, 257)], axis=1).astype(np.float32)
    ref, tgt = tof.texture(w, h), tof.texture(w, h, shift)
    m = ofm.Tracker(w, h)
    m.set_reference(ref)
    return ref, tgt, pts, m.track(tgt, pts)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_point_counts(n):
    from dsopp_amd import capi
    ref, tgt, pts, want = _many_points_case()
    t = capi.OpticalFlowTracker(161, 123)
    t.set_reference(ref)
    got = t.track(tgt, pts[:n], with_iterations=True)
    assert got[0].shape == (n, 2) and got[3].shape == (n, t.num_levels)
    _assert_track(got, tuple(a[:n] for a in want), f"n = {n}")
    t.close()


@pytest.mark.parametrize("options", [dict(window=5, max_level=0), dict(max_iterations=0), dict(window=9, max_level=5, epsilon=0.3, min_eig_threshold=1e-2)])
def test_other_options(options):
    from dsopp_amd import capi
    ref, tgt, pts, _ = _many_points_case()
    pts = pts[:70]
    m = ofm.Tracker(161, 123, **options)
    m.set_reference(ref)
    want = m.track(tgt, pts)
    t = capi.OpticalFlowTracker(161, 123, **options)
    assert t.num_levels == m.n_levels
    t.set_reference(ref)
    got = t.track(tgt, pts, with_iterations=True)
    _assert_track(got, want, str(options))
    if options.get("max_iterations") == 0:
        assert np.all(got[3] == 0)
    t.close()


def test_repeated_and_interleaved_calls():
    """the same call twice gives the same bytes, and the reference survives a track() of another frame"""
    from dsopp_amd import capi
    ref, tgt, pts, want = _random_case()
    other = tof.texture(161, 123)
    t = capi.OpticalFlowTracker(161, 123)
    t.set_reference(ref)
    first = t.track(tgt, pts, with_iterations=True)
    second = t.track(tgt, pts, with_iterations=True)
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()
    m = ofm.Tracker(161, 123)
    m.set_reference(ref)
    _assert_track(t.track(other, pts, with_iterations=True), m.track(other, pts), "another target")
    _assert_track(t.track(tgt, pts, with_iterations=True), want, "the first target again")
    t.close()


def test_guard_bytes_behind_every_output():
    from dsopp_amd import capi
    ref, tgt, pts, want = _random_case()
    n, guard = len(pts), 64
    t = capi.OpticalFlowTracker(161, 123)
    t.set_reference(ref)
    sizes = {"to": 8 * n, "status": n, "err": 4 * n, "iterations": 4 * n * t.num_levels}
    bufs = {k: np.full(v + guard, 0xA5, np.uint8) for k, v in sizes.items()}
    src = np.ascontiguousarray(pts)
    capi._chk(capi.lib().dsopp_hip_flow_tracker_track(t._h, capi._p(tgt, np.uint8), C.c_size_t(161), n, capi._p(src, np.float32), capi._p(bufs["to"], np.uint8),
                                                      capi._p(bufs["status"], np.uint8), capi._p(bufs["err"], np.uint8), capi._p(bufs["iterations"], np.uint8)))
    for k, v in sizes.items():
        assert np.all(bufs[k][v:] == 0xA5), k
    got = (bufs["to"][:8 * n].view(np.float32).reshape(n, 2), bufs["status"][:n], bufs["err"][:4 * n].view(np.float32),
           bufs["iterations"][:sizes["iterations"]].view(np.int32).reshape(n, t.num_levels))
    _assert_track(got, want, "guarded outputs")
    t.close()


def test_error_codes():
    from dsopp_amd import capi
    img, pts = tof.texture(64, 48), np.array([[30.0, 20.0]], np.float32)
    t = capi.OpticalFlowTracker(64, 48)
    with pytest.raises(capi.HipError, match="error -6"):       # DSOPP_HIP_ERR_STATE: no reference yet
        t.track(img, pts)
    with pytest.raises(capi.HipError, match="error -6"):
        t.get_level(0, 0)
    for bad in (dict(window=14), dict(window=17), dict(window=1), dict(max_level=6), dict(max_level=-1)):
        with pytest.raises(capi.HipError, match="error -1"):
            capi.OpticalFlowTracker(64, 48, **bad)
    with pytest.raises(capi.HipError, match="error -1"):
        capi.OpticalFlowTracker(1, 48)
    p = capi.Pyramid(80, 48, 1)
    p.build_undistorted(capi.Undistorter((80, 48), (80, 48)), tof.texture(80, 48))
    with pytest.raises(capi.HipError, match="error -1"):       # another size
        t.set_reference(p)
    q = capi.Pyramid(64, 48, 1)
    q.build(img)
    with pytest.raises(capi.HipError, match="error -6"):       # a plain build keeps no 8-bit image
        t.set_reference(q)
    t.set_reference(img)
    with pytest.raises(capi.HipError, match="error -1"):
        t.track(p, pts)
    with pytest.raises(capi.HipError, match="error -6"):
        t.track(q, pts)
    to, status, err = t.track(img, pts)                        # and the object still works
    assert status[0] == 1 and np.array_equal(to, pts)
    for o in (t, p, q):
        o.close()


def test_host_mirror_prints_the_python_result(tmp_path):
    from dsopp_amd import capi
    ref, tgt, pts, want = _random_case()
    path = tmp_path / "flow_case.bin"
    with open(path, "wb") as f:
        f.write(b"161 123 %d\n" % len(pts))
        f.write(ref.tobytes() + tgt.tobytes() + pts.tobytes())
    exe = tof.build_example(tmp_path)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    t = capi.OpticalFlowTracker(161, 123)
    t.set_reference(ref)
    to, status, err = t.track(tgt, pts)
    t.close()
    lines = r.stdout.strip().splitlines()
    kept = np.flatnonzero(status)
    assert lines[0] == f"correspondences {len(kept)} of {len(pts)}" and len(lines) == 1 + len(kept)
    for k, (i, line) in enumerate(zip(kept, lines[1:])):
        assert line == "%d %d %08x %08x %08x" % (i, k, _bits(to[i])[0], _bits(to[i])[1], _bits(err[i:i + 1])[0])
