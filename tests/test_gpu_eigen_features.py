"""The device's eigen tracking-feature extractor (dsopp_hip_feature_extractor_create_eigen, features_eigen.hip) against the NumPy
model of tests/eigen_features_model.py, bit for bit: lists, counts, state and pass statistics are integers, so there is no tolerance
anywhere.  Frames are rendered scenes of dsopp_amd/synthetic.py rounded and clipped to u8 as the tick sequence does; masks have the
shapes of test_gpu_features.py."""
import functools

import numpy as np
import pytest

import eigen_features_model as em
import features_model as fm
from dsopp_amd import synthetic as syn

pytestmark = pytest.mark.gpu

SIZES = {"640x480": (640, 480), "1280x1024": (1280, 1024), "643x481": (643, 481)}
MASKS = ("none", "pixel", "band")
ERR_INVALID_ARGUMENT, ERR_CAPACITY, ERR_STATE = -1, -5, -6


def _mask(kind, H, W, seed):
    if kind == "none":
        return None
    rng = np.random.default_rng(seed)
    if kind == "pixel":
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
    T = syn.se3_exp(np.array([0.03 * i, -0.01 * i, 0.02 * i, 0.002 * i, -0.003 * i, 0.001 * i]))
    img, _ = _scene(W, H).render_torch(T, 0.02 * i, 1.5 * i, "cuda")
    return np.clip(np.round(img), 0, 255).astype(np.uint8)


def constant_rows(W, H, seed=3):
    """every row one value: dx = 0 everywhere, so direction 8 (1, 0) projects every gradient to exactly 0"""
    rng = np.random.default_rng(seed)
    rows = np.clip(np.cumsum(rng.integers(-9, 10, H)) + 128, 0, 255)
    return np.repeat(rows[:, None], W, axis=1).astype(np.uint8)


def smooth_ramp(W, H):
    """gradients far below the level-0 threshold: only the coarse levels see enough of the slope"""
    ys, xs = np.mgrid[0:H, 0:W]
    return np.clip(np.round(20 + 0.2 * xs + 0.15 * ys), 0, 255).astype(np.uint8)


def _pair(W, H, density, **kw):
    from dsopp_amd import capi
    return capi.EigenFeatureExtractor(W, H, density, **kw), em.EigenExtractorModel(W, H, density)


def _check(ex, model, img, mask, what):
    got, want = ex.extract(img, mask), model.extract(img, mask)
    assert got.shape == want.shape and np.array_equal(got, want), (what, got.shape, want.shape)
    assert ex.state() == model.state(), (what, ex.state(), model.state())
    st = ex.stats()
    assert {k: st[k] for k in ("passes", "potentials", "found")} == model.stats, (what, st, model.stats)
    return got, st


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("size", SIZES)
def test_extract_matches_model(size, kind):
    W, H = SIZES[size]
    mask = _mask(kind, H, W, 5)
    density = 2000.0 if W > 1000 else 1500.0
    ex, model = _pair(W, H, density)
    try:
        for i in range(1 if W > 1000 else 2):
            got, _ = _check(ex, model, _frame(W, H, i), mask, (size, kind, i))
            assert len(got) > 100
    finally:
        ex.close()


@pytest.mark.parametrize("density", [150.0, 3000.0])
def test_sequence_adapts_like_the_model(density):
    """six frames on one extractor: the window size moves (up for a low density, down for a high one) and every call matches"""
    W, H = SIZES["640x480"]
    ex, model = _pair(W, H, density)
    potentials = []
    try:
        for i in range(6):
            _check(ex, model, _frame(W, H, i), None, (density, i))
            potentials.append(ex.state()["window_size"])
        if density < 1000:
            assert potentials[0] > em.INITIAL_POTENTIAL
        else:
            assert potentials[0] < em.INITIAL_POTENTIAL
    finally:
        ex.close()


def test_constant_rows_are_walked_in_order():
    """dx = 0 everywhere: emission counts depend on the directions, the undetermined top windows are chained, the list still matches"""
    W, H = 320, 240
    ex, model = _pair(W, H, 800.0)
    try:
        img = constant_rows(W, H)
        _check(ex, model, img, None, "constant rows")
        assert ex.stats()["chained_windows"] > 0
    finally:
        ex.close()


def test_smooth_ramp_emits_on_coarse_levels():
    W, H = 640, 480
    ex, model = _pair(W, H, 7.0)   # one pass at the initial window size
    try:
        got, _ = _check(ex, model, smooth_ramp(W, H), None, "ramp")
        assert len(got) > 0 and min(level for _, level in model.last_features) >= 2
    finally:
        ex.close()


def test_flat_image_finds_nothing():
    """found == 0: ratio = inf, the window size drops to 1 for the second pass, which finds nothing either"""
    W, H = 192, 160
    ex, model = _pair(W, H, 300.0)
    try:
        flat = np.full((H, W), 128, dtype=np.uint8)
        got, st = _check(ex, model, flat, None, "flat")
        assert len(got) == 0 and st["found"] == [0, 0] and st["passes"] == 2 and ex.state()["window_size"] == 1
        _check(ex, model, _frame(640, 480, 0)[100:100 + H, 200:200 + W].copy(), None, "after flat")
    finally:
        ex.close()


def test_capacity_too_small_reports_and_keeps_the_state():
    W, H = 640, 480
    ex, model = _pair(W, H, 1500.0)
    try:
        img = _frame(W, H, 0)
        before = ex.state()
        rc, _, n = ex.extract_raw(img, 10)
        assert rc == ERR_CAPACITY and ex.state() == before and not before["initialized"]
        want = model.extract(img)
        assert n == len(want)
        rc, got, n2 = ex.extract_raw(img, n)
        assert rc == 0 and n2 == n and np.array_equal(got, want)
        assert ex.state() == model.state()
    finally:
        ex.close()


def test_bad_arguments_are_refused():
    from dsopp_amd import capi
    for W, H, d in ((31, 64, 100.0), (64, 31, 100.0), (64, 64, 0.0), (64, 64, -1.0)):
        with pytest.raises(capi.HipError):
            capi.EigenFeatureExtractor(W, H, d)
    sobel = capi.FeatureExtractor(64, 64)
    try:
        with pytest.raises(capi.HipError, match=f"error {ERR_STATE}"):
            capi.EigenFeatureExtractor.stats(sobel)
    finally:
        sobel.close()
    ex = capi.EigenFeatureExtractor(32, 32, 50.0)   # the smallest size: a 1 x 1 threshold map
    try:
        img = _frame(640, 480, 1)[200:232, 300:332].copy()
        m = em.EigenExtractorModel(32, 32, 50.0)
        assert np.array_equal(ex.extract(img), m.extract(img)) and ex.state() == m.state()
    finally:
        ex.close()


def test_two_streams_and_interleaved_sobel():
    """two eigen extractors on two streams and a Sobel extractor sharing the first stream, called in turns: each matches its model"""
    import torch
    from dsopp_amd import capi
    W, H = SIZES["643x481"]
    mask = _mask("band", H, W, 9)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a = capi.EigenFeatureExtractor(W, H, 1500.0, stream=s1.cuda_stream)
    b = capi.EigenFeatureExtractor(W, H, 800.0, stream=s2.cuda_stream)
    c = capi.FeatureExtractor(W, H, 1500.0, 0.6, stream=s1.cuda_stream)
    ma, mb = em.EigenExtractorModel(W, H, 1500.0), em.EigenExtractorModel(W, H, 800.0)
    mc = fm.SobelExtractorModel(W, H, 1500.0, 0.6, capi.features_shuffle_order)
    try:
        for i in range(2):
            img = _frame(W, H, i)
            ga, gc, gb = a.extract(img, mask), c.extract(img, mask), b.extract(img)
            assert np.array_equal(ga, ma.extract(img, mask)) and a.state() == ma.state(), i
            assert np.array_equal(gc, mc.extract(img, mask)), i
            assert np.array_equal(gb, mb.extract(img)) and b.state() == mb.state(), i
    finally:
        a.close()
        b.close()
        c.close()


@pytest.mark.parametrize("f32", [False, True])
def test_immature_set_from_eigen_features(f32):
    from dsopp_amd import capi
    W, H = SIZES["640x480"]
    img = _frame(W, H, 2)
    ex, model = _pair(W, H, 1500.0)
    pyr = capi.Pyramid(W, H, 1, dtype=capi.F32 if f32 else capi.F64)
    try:
        xy = ex.extract(img)
        assert np.array_equal(xy, model.extract(img))
        pyr.build(img)
        intr = _scene(W, H).intrinsics
        s = capi.ImmatureSet.from_features(ex, pyr, intr)
        try:
            want = fm.immature_inputs(xy, pyr.get_level(0), intr, f32=f32)
            got = s.inputs()
            assert s.n == len(want["projection"]) > 0
            for k in ("projection", "direction", "patch", "gradient"):
                assert np.array_equal(got[k], want[k]), k
        finally:
            s.close()
    finally:
        ex.close()
        pyr.close()
