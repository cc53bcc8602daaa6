"""The device's Sobel tracking-feature extractor (dsopp_hip_feature_extractor, features.hip) and the immature-landmark build
from its list (dsopp_hip_immature_set_create_from_features) against the NumPy model of tests/features_model.py, bit for bit:
the lists are integers, so there is no tolerance anywhere.  Frames are rendered scenes of dsopp_amd/synthetic.py rounded and
clipped to u8 as the tick sequence does; masks have the shapes of test_gpu_masks.py."""
import functools

import numpy as np
import pytest

import features_model as fm
from dsopp_amd import synthetic as syn

pytestmark = pytest.mark.gpu

SIZES = {"640x480": (640, 480), "1280x1024": (1280, 1024), "643x481": (643, 481)}
MASKS = ("none", "pixel", "band")
ERR_CAPACITY = -5


def _mask(kind, H, W, seed):
    if kind == "none":
        return None
    rng = np.random.default_rng(seed)
    if kind == "pixel":   # sparser than test_gpu_masks.py's 15 %: the 15 x 15 erosion must leave pixels to find
        return (rng.random((H, W)) >= 0.002).astype(np.uint8) * 255
    m = np.full((H, W), 255, dtype=np.uint8)
    m[int(0.55 * H):int(0.55 * H) + 9, :] = 0
    m[:, int(0.3 * W):int(0.3 * W) + 5] = 0
    for _ in range(12):
        y, x = rng.integers(0, H - 20), rng.integers(0, W - 20)
        m[y:y + rng.integers(3, 20), x:x + rng.integers(3, 20)] = 0
    return m


@functools.lru_cache(maxsize=None)
def _scene(W, H):
    return syn.Scene.make(W, H, seed=11)


@functools.lru_cache(maxsize=None)
def _frame(W, H, i):
    """frame i of a short camera path through the scene, as u8 (scripts/tick_sequence.py: round, clip)"""
    T = syn.se3_exp(np.array([0.03 * i, -0.01 * i, 0.02 * i, 0.002 * i, -0.003 * i, 0.001 * i]))
    img, _ = _scene(W, H).render_torch(T, 0.02 * i, 1.5 * i, "cuda")
    return np.clip(np.round(img), 0, 255).astype(np.uint8)


def _pair(W, H, density=1500.0, q=0.6, **kw):
    from dsopp_amd import capi
    return capi.FeatureExtractor(W, H, density, q, **kw), fm.SobelExtractorModel(W, H, density, q, capi.features_shuffle_order)


def _same_state(ex, model, what):
    got, want = ex.state(), model.state()
    assert got == want, (what, got, want)


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("size", SIZES)
def test_extract_matches_model(size, kind):
    """first call (threshold from the histogram, window size) and one adaptation, with and without a camera mask"""
    W, H = SIZES[size]
    mask = _mask(kind, H, W, 5)
    ex, model = _pair(W, H)
    try:
        for i in range(2):
            img = _frame(W, H, i)
            got, want = ex.extract(img, mask), model.extract(img, mask)
            assert got.shape == want.shape and np.array_equal(got, want), (size, kind, i, got.shape, want.shape)
            _same_state(ex, model, (size, kind, i))
        if mask is not None:   # the mask must matter: the same frame without it gives another list
            assert not np.array_equal(fm.SobelExtractorModel(W, H, 1500.0, 0.6, lambda n: np.arange(n)).extract(img, None),
                                      fm.SobelExtractorModel(W, H, 1500.0, 0.6, lambda n: np.arange(n)).extract(img, mask))
    finally:
        ex.close()


@pytest.mark.parametrize("density", [500.0, 1500.0, 3000.0])
def test_sequence_adapts_like_the_model(density):
    """seven calls on one extractor with different frames: the state equals the model's after every call, and the truncation runs"""
    W, H = SIZES["640x480"]
    ex, model = _pair(W, H, density)
    truncated = 0
    try:
        for i in range(7):
            img = _frame(W, H, i)
            got, want = ex.extract(img), model.extract(img)
            assert np.array_equal(got, want), (density, i, got.shape, want.shape)
            _same_state(ex, model, (density, i))
            truncated += model.found_last > density
        assert truncated > 0 and model.window_size == int(np.sqrt(W * H * 0.4 / density))
    finally:
        ex.close()


def test_window_size_one_compacts_every_pixel_window():
    """a density above W * H * (1 - q): the first call lowers it, the window size is 1 and every pixel is a window"""
    W, H = 96, 64
    img = _frame(640, 480, 2)[100:100 + H, 200:200 + W].copy()
    ex, model = _pair(W, H, 1e5)
    try:
        for i in range(3):
            frame = img if i == 0 else _frame(640, 480, 2 + i)[100:100 + H, 200:200 + W].copy()
            got, want = ex.extract(frame), model.extract(frame)
            assert np.array_equal(got, want), i
            _same_state(ex, model, i)
        assert model.window_size == 1 and model.density < W * H
        assert model.found_last > 1000   # most of the (W - 1) * (H - 1) windows hit
    finally:
        ex.close()


def test_flat_image_finds_nothing_and_keeps_the_threshold():
    """found == 0 (the reference divides by zero there): no feature, no fault, the threshold as it was"""
    W, H = 640, 480
    flat = np.full((H, W), 128, dtype=np.uint8)
    ex, model = _pair(W, H)
    try:   # after an adapting call
        img = _frame(W, H, 0)
        assert np.array_equal(ex.extract(img), model.extract(img))
        thr = ex.state()["grad_norm_threshold"]
        assert thr > 0
        assert len(ex.extract(flat)) == 0 and len(model.extract(flat)) == 0
        _same_state(ex, model, "flat later")
        assert ex.state()["grad_norm_threshold"] == thr and ex.state()["found_last"] == 0
        img = _frame(W, H, 1)
        assert np.array_equal(ex.extract(img), model.extract(img))
    finally:
        ex.close()
    ex, model = _pair(W, H)
    try:   # as the first call: the quantile of an all-zero norm is 0
        assert len(ex.extract(flat)) == 0 and len(model.extract(flat)) == 0
        _same_state(ex, model, "flat first")
        assert ex.state()["initialized"] and ex.state()["grad_norm_threshold"] == 0
    finally:
        ex.close()


def test_capacity_too_small_reports_and_keeps_the_state():
    W, H = 640, 480
    ex, model = _pair(W, H)
    try:
        img = _frame(W, H, 0)
        before = ex.state()
        rc, _, n = ex.extract_raw(img, 10)
        assert rc == ERR_CAPACITY and ex.state() == before and not before["initialized"]
        want = model.extract(img)
        assert n == len(want)
        rc, got, n2 = ex.extract_raw(img, n)
        assert rc == 0 and n2 == n and np.array_equal(got, want)
        _same_state(ex, model, "after capacity")
        st = ex.state()
        img1 = _frame(W, H, 1)
        rc, _, n = ex.extract_raw(img1, 0)
        assert rc == ERR_CAPACITY and ex.state() == st
        assert np.array_equal(ex.extract(img1), model.extract(img1))
        _same_state(ex, model, "second call")
    finally:
        ex.close()


def test_two_extractors_on_two_streams_agree():
    import torch
    from dsopp_amd import capi
    W, H = SIZES["643x481"]
    mask = _mask("band", H, W, 9)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a = capi.FeatureExtractor(W, H, stream=s1.cuda_stream)
    b = capi.FeatureExtractor(W, H, stream=s2.cuda_stream)
    try:
        for i in range(3):
            img = _frame(W, H, i)
            assert np.array_equal(a.extract(img, mask), b.extract(img, mask)), i
            assert a.state() == b.state()
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("size", ["640x480", "643x481"])
def test_immature_set_from_features_matches_model(size, dtype):
    """buildFeatures + pushImmatureLandmarks on the device: inputs() equal the model's step 7 over the pyramid's own level 0"""
    from dsopp_amd import capi
    W, H = SIZES[size]
    scene = _scene(W, H)
    intr = scene.intrinsics
    ex, model = _pair(W, H)
    pyr = capi.Pyramid(W, H, 1, capi.F64 if dtype == "f64" else capi.F32)
    try:
        for i in range(2):
            img = _frame(W, H, i)
            xy = ex.extract(img)
            assert np.array_equal(xy, model.extract(img))
            pyr.build(img)
            s = capi.ImmatureSet.from_features(ex, pyr, intr)
            try:
                want = fm.immature_inputs(xy, pyr.get_level(0), intr, f32=dtype == "f32")
                got = s.inputs()
                assert s.n == len(want["projection"]) and s.n < len(xy)   # ROI drops happened
                for k in want:
                    assert np.array_equal(got[k], want[k]), (size, dtype, i, k)
                near_edge = (xy[:, 0] < 4) | (xy[:, 1] < 4) | (xy[:, 0] > W - 5) | (xy[:, 1] > H - 5)
                assert near_edge.sum() == len(xy) - s.n
                st = s.download()
                assert (st["status"] == syn.IMMATURE_STATUS["uninitialized"]).all() and (st["idepth_max"] == 1.0 / 0.001).all()
            finally:
                s.close()
    finally:
        ex.close()
        pyr.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_set_from_features_estimates_like_a_host_built_set(dtype):
    """a set built on the device and one created from its downloaded inputs give the same depth-estimation state"""
    from dsopp_amd import capi
    W, H = SIZES["640x480"]
    scene = _scene(W, H)
    intr = scene.intrinsics
    F = capi.F64 if dtype == "f64" else capi.F32
    ex = capi.FeatureExtractor(W, H)
    ref, tgt = capi.Pyramid(W, H, 1, F), capi.Pyramid(W, H, 1, F)
    try:
        img = _frame(W, H, 0)
        ex.extract(img)
        ref.build(img)
        dev = capi.ImmatureSet.from_features(ex, ref, intr)
        inp = dev.inputs()
        host = capi.ImmatureSet(syn.new_immature_landmarks(inp["projection"], inp["direction"], inp["patch"], inp["gradient"]))
        T_wt = syn.se3_exp(np.array([0.03, -0.01, 0.02, 0.002, -0.003, 0.001]))
        tgt.build(_frame(W, H, 1))
        Tp = syn.mat_to_params(np.linalg.inv(T_wt))
        for s in (dev, host):
            s.estimate(tgt, 0, intr, Tp, 1.0, (0.0, 0.0), 1.0, (0.02, 1.5))
        a, b = dev.download(), host.download()
        for k in a:
            assert np.array_equal(a[k], b[k]), k
        assert (a["status"] != syn.IMMATURE_STATUS["uninitialized"]).any()
        dev.close()
        host.close()
    finally:
        ex.close()
        ref.close()
        tgt.close()
