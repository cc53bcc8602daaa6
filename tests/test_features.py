"""The NumPy model of the Sobel tracking-feature extractor (tests/features_model.py) pinned on hand-checked cases, and the
reference's shuffle order as the library reports it (dsopp_hip_features_shuffle_order: no device needed).  What the GPU tests
(test_gpu_features.py) hold the device to is only as good as this model."""
import math

import numpy as np
import pytest

import features_model as fm


def _sobel_by_hand(img):
    """|Sx| + |Sy| pixel by pixel, the 3x3 sums written out, reflect-101 borders spelled as index rules"""
    H, W = img.shape
    p = img.astype(np.int64)

    def at(y, x):
        y = 1 if y == -1 else (H - 2 if y == H else y)
        x = 1 if x == -1 else (W - 2 if x == W else x)
        return p[y, x]

    out = np.zeros((H, W), dtype=np.int64)
    for y in range(H):
        for x in range(W):
            sx = (-at(y - 1, x - 1) + at(y - 1, x + 1) - 2 * at(y, x - 1) + 2 * at(y, x + 1) - at(y + 1, x - 1) + at(y + 1, x + 1))
            sy = (-at(y - 1, x - 1) - 2 * at(y - 1, x) - at(y - 1, x + 1) + at(y + 1, x - 1) + 2 * at(y + 1, x) + at(y + 1, x + 1))
            out[y, x] = abs(sx) + abs(sy)
    return out


@pytest.mark.parametrize("shape", [(2, 2), (3, 2), (2, 3), (3, 3), (5, 7), (16, 17)])
def test_sobel_matches_hand_sums_on_every_border(shape):
    rng = np.random.default_rng(sum(shape))
    img = rng.integers(0, 256, shape).astype(np.uint8)
    g = fm.sobel_norm(img)
    assert g.dtype == np.int16
    np.testing.assert_array_equal(g, _sobel_by_hand(img))


def test_sobel_hand_values():
    # a vertical step 0 | 255: the column next to it sees Sx = 4 * 255, the border column reflects onto itself (Sx = 0)
    img = np.zeros((4, 4), dtype=np.uint8)
    img[:, 2:] = 255
    g = fm.sobel_norm(img)
    assert g[1, 1] == 4 * 255 and g[1, 2] == 4 * 255 and g[1, 0] == 0 and g[1, 3] == 0
    # W = 2: x - 1 and x + 1 both read the other column, so Sx is 0 everywhere; H = 3: rows 0 and 2 reflect onto row 1, so Sy is 0 there
    img2 = np.array([[0, 9], [3, 200], [7, 1]], dtype=np.uint8)
    g2 = fm.sobel_norm(img2)
    assert g2[0].tolist() == [0, 0] and g2[2].tolist() == [0, 0]
    # row 1, x = 0: Sy = (1 + 2 * 7 + 1) - (9 + 2 * 0 + 9) = -2; x = 1: Sy = (7 + 2 * 1 + 7) - (0 + 2 * 9 + 0) = -2
    assert g2[1].tolist() == [2, 2]


def _valid_by_hand(mask):
    H, W = mask.shape
    out = np.zeros((H, W), dtype=bool)
    for y in range(H):
        for x in range(W):
            out[y, x] = bool(np.all(mask[max(0, y - 7):y + 8, max(0, x - 7):x + 8] != 0))
    return out


def test_erosion_single_interior_zero():
    m = np.full((40, 50), 255, dtype=np.uint8)
    m[20, 25] = 0
    v = fm.eroded_valid(m, m.shape)
    ys, xs = np.nonzero(~v)
    assert (ys.min(), ys.max(), xs.min(), xs.max()) == (13, 27, 18, 32)   # a 15 x 15 square around it
    np.testing.assert_array_equal(v, _valid_by_hand(m))


def test_erosion_corner_zero_and_edge_does_not_erode():
    m = np.full((30, 30), 1, dtype=np.uint8)
    m[0, 0] = 0
    v = fm.eroded_valid(m, m.shape)
    assert not v[:8, :8].any() and v[8, 0] and v[0, 8] and v[8:, :].all()
    # all-valid mask: nothing erodes, the image edge included
    assert fm.eroded_valid(np.ones((20, 20), np.uint8), (20, 20)).all()
    assert fm.eroded_valid(None, (5, 6)).all()


@pytest.mark.parametrize("dist", [7, 8])
def test_erosion_zero_near_the_edge(dist):
    """a zero 7 or 8 px from the left edge: it erodes x in [dist - 7, dist + 7], so the edge column is reached only from 7 px"""
    m = np.full((31, 40), 255, dtype=np.uint8)
    m[15, dist] = 0
    v = fm.eroded_valid(m, m.shape)
    assert v[15, 0] == (dist > 7)
    assert not v[15, dist + 7] and v[15, dist + 8]
    np.testing.assert_array_equal(v, _valid_by_hand(m))


def test_random_mask_erosion_matches_the_box_rule():
    rng = np.random.default_rng(4)
    m = (rng.random((37, 45)) > 0.01).astype(np.uint8) * 255
    np.testing.assert_array_equal(fm.eroded_valid(m, m.shape), _valid_by_hand(m))


def test_quantile_index():
    assert fm.quantile_index(1280 * 1024, 0.6) == 786432
    assert fm.quantile_index(640 * 480, 0.6) == int(307200 * 0.6)
    g = np.arange(10, dtype=np.int16)[::-1].copy()
    k = fm.quantile_index(g.size, 0.6)
    assert np.partition(g, k)[k] == 6


def test_threshold_update_int_division():
    # 307200 / 1500 = 204 (int), 307200 / 2000 = 153: thr * log(204) / log(153)
    assert fm.updated_threshold(307200, 1500, 2000, 100) == int(100 * math.log(204) / math.log(153))
    # the divisions are integer ones: 1000 / 3 = 333, not 333.33
    assert fm.updated_threshold(1000, 3, 7, 50) == int(50 * math.log(333) / math.log(142))
    # the quotient is truncated toward zero: 37 * log(384) / log(102) = 47.61...
    assert fm.updated_threshold(307200, 800, 3000, 37) == 47


def test_threshold_update_undefined_cases_keep_the_threshold():
    assert fm.updated_threshold(307200, 1500, 0, 123) == 123        # found == 0: division by zero in the reference
    assert fm.updated_threshold(307200, 0, 10, 77) == 77            # desired == 0 (density below 1)
    assert fm.updated_threshold(300, 1, 200, 55) == 55              # 300 / 200 = 1: log(1) = 0, non-finite quotient
    assert fm.updated_threshold(300, 300, 200, 55) == 55            # 0 / 0
    assert fm.updated_threshold(300, 300, 100, 55) == 0             # log(1) / log(3): finite


def test_window_scan_rules():
    """windows start while start + ws < size (the last partial window is skipped); the first hit in raster order wins"""
    g = np.zeros((10, 10), dtype=np.int16)
    g[0, 2] = g[1, 0] = 50      # window (0, 0) with ws = 3: raster order picks (x 2, y 0), not (x 0, y 1)
    g[9, 9] = 50                # last row / column: never scanned (9 + 3 >= 10)
    g[7, 8] = 50                # window (2, 2) covers 6..8
    hits = fm.window_hits(g, np.ones_like(g, dtype=bool), 10, 3)
    assert hits.tolist() == [0 * 10 + 2, 7 * 10 + 8]
    assert fm.window_hits(g, np.ones_like(g, dtype=bool), 50, 3).tolist() == []    # strict >


def test_model_first_call_and_truncation():
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (48, 64)).astype(np.uint8)
    from dsopp_amd import capi
    m = fm.SobelExtractorModel(64, 48, 20.0, 0.6, capi.features_shuffle_order)
    xy = m.extract(img)
    st = m.state()
    assert st["initialized"] and st["window_size"] == int(math.sqrt(64 * 48 * 0.4 / 20.0))
    assert st["found_last"] > 20 and len(xy) == 20       # truncated to (long)density
    # ws = 1: a density above W * H * (1 - q) is lowered to it
    m1 = fm.SobelExtractorModel(64, 48, 5000.0, 0.6, capi.features_shuffle_order)
    m1.extract(img)
    assert m1.window_size == 1 and m1.density == pytest.approx(64 * 48 * 0.4)


def test_shuffle_order_fingerprints():
    """std::shuffle(iota(n), std::default_random_engine{}) of libstdc++, as the reference applies it"""
    from dsopp_amd import capi
    assert capi.features_shuffle_order(10).tolist() == [2, 7, 1, 6, 8, 0, 4, 9, 5, 3]
    assert capi.features_shuffle_order(1000)[:10].tolist() == [502, 870, 164, 770, 786, 944, 562, 820, 438, 328]
    p = capi.features_shuffle_order(60000)
    assert p[:10].tolist() == [7657, 15610, 58593, 37701, 54512, 46264, 3290, 40083, 10870, 22316]
    assert np.array_equal(np.sort(p), np.arange(60000))
    assert capi.features_shuffle_order(0).tolist() == [] and capi.features_shuffle_order(1).tolist() == [0]


def test_feature_extractor_argument_checks():
    """bad sizes, densities and quantile levels are refused before any device is touched"""
    import ctypes as C
    from dsopp_amd import capi
    lib = capi.lib()
    h = C.c_void_p()
    for w, h_, d, q in [(15, 64, 1500.0, 0.6), (64, 15, 1500.0, 0.6), (64, 64, 0.0, 0.6), (64, 64, -1.0, 0.6), (64, 64, 1500.0, 0.0),
                        (64, 64, 1500.0, 1.0), (64, 64, 1500.0, float("nan"))]:
        assert lib.dsopp_hip_feature_extractor_create(0, None, w, h_, C.c_double(d), C.c_double(q), C.byref(h)) == -1, (w, h_, d, q)
    assert lib.dsopp_hip_features_shuffle_order(-1, None) == -1


def test_feature_extractor_no_cpu_fallback():
    """without a device the extractor fails with DSOPP_HIP_ERR_HIP"""
    from dsopp_amd import capi
    if capi.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(capi.HipError) as e:
        capi.FeatureExtractor(64, 48)
    assert "-4" in str(e.value)
