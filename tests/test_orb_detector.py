"""tests/orb_model.py, the NumPy statement of the device ORB keypoint detector (include/dsopp_hip.h, dsopp_hip_orb_detector_create), pinned on
literal restatements of its steps and on hand cases; tests/test_gpu_orb_detector.py holds the device to the model.  Only the
features-per-level case and the driver's build need the library; none needs a device."""
import os
import subprocess

import numpy as np
import pytest

import orb_model as om

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
BACKGROUND = 50


def texture(width, height, cell=8, seed=1, margin=0):
    """random cells of `cell` pixels plus noise of +-6: corners on every level, which white noise does not have above level 0"""
    rng = np.random.default_rng(seed)
    w, h = width + margin, height + margin
    cells = rng.integers(0, 256, ((h + cell - 1) // cell, (w + cell - 1) // cell))
    img = np.kron(cells, np.ones((cell, cell), np.int64))[:h, :w] + rng.integers(-6, 7, (h, w))
    return np.clip(img, 0, 255).astype(np.uint8)


def dots(width, height, points):
    """isolated pixels (x, y, value) on a flat background"""
    img = np.full((height, width), BACKGROUND, np.uint8)
    for x, y, v in points:
        img[y, x] = v
    return img


def ring_patch(centre, ring_values):
    p = np.full((7, 7), centre, np.uint8)
    for (dx, dy), v in zip(om.RING, ring_values):
        p[3 + dy, 3 + dx] = v
    return p


def literal_corner(patch, t):
    """FAST-9/16 as a sentence: 9 contiguous ring pixels all brighter than v + t or all darker than v - t"""
    v = int(patch[3, 3])
    ring = [int(patch[3 + dy, 3 + dx]) for dx, dy in om.RING]
    for start in range(16):
        arc = [ring[(start + k) % 16] for k in range(9)]
        if all(p > v + t for p in arc) or all(p < v - t for p in arc):
            return True
    return False


def test_fast_score_is_the_largest_threshold_that_still_gives_a_corner():
    rng = np.random.default_rng(7)
    seen_corner = seen_none = 0
    for _ in range(300):
        v = int(rng.integers(0, 256))
        ring = v + rng.integers(-12, 13, 16)
        start, length, sign = int(rng.integers(0, 16)), int(rng.integers(6, 13)), int(rng.choice((-1, 1)))
        for k in range(length):
            ring[(start + k) % 16] = v + sign * int(rng.integers(15, 90))
        patch = np.clip(rng.integers(0, 256, (7, 7)), 0, 255).astype(np.uint8)
        patch[3, 3] = v
        for (dx, dy), value in zip(om.RING, np.clip(ring, 0, 255)):
            patch[3 + dy, 3 + dx] = value
        passing = [t for t in range(256) if literal_corner(patch, t)]
        for threshold in (0, 20, 40):
            want = max(passing) if passing and max(passing) >= threshold else 0
            assert om.fast_scores(patch, threshold)[3, 3] == want
        seen_corner += bool(passing and max(passing) >= 20)
        seen_none += not passing
    assert seen_corner > 50 and seen_none > 20


def test_fast_hand_cases():
    # an isolated pixel of value v on background g scores v - g - 1, darker or brighter
    for v, g in ((200, 50), (30, 90)):
        img = np.full((15, 15), g, np.uint8)
        img[7, 7] = v
        s = om.fast_scores(img, 20)
        assert s[7, 7] == abs(v - g) - 1 and np.count_nonzero(s) == 1
    # a ring difference of exactly t is no corner, t + 1 scores t
    t = 20
    assert om.fast_scores(ring_patch(100, [100 + t] * 16), t)[3, 3] == 0
    assert om.fast_scores(ring_patch(100, [100 + t + 1] * 16), t)[3, 3] == t
    assert om.fast_scores(ring_patch(100, [100 - t] * 16), t)[3, 3] == 0
    assert om.fast_scores(ring_patch(100, [100 - t - 1] * 16), t)[3, 3] == t
    # an arc of 8 is no corner, an arc of 9 is one, wherever it starts: the arcs from 8 on wrap ring index 15 -> 0
    for start in range(16):
        for length, corner in ((8, False), (9, True)):
            ring = [100] * 16
            for k in range(length):
                ring[(start + k) % 16] = 160
            assert (om.fast_scores(ring_patch(100, ring), t)[3, 3] == 59) == corner
            assert (om.fast_scores(ring_patch(100, ring), t)[3, 3] != 0) == corner
    # centres closer than 3 pixels to the border score 0
    img = dots(12, 12, [(2, 6, 200), (6, 2, 200), (9, 6, 200), (6, 9, 200), (3, 3, 200), (8, 8, 200)])
    s = om.fast_scores(img, t)
    assert sorted(zip(*np.nonzero(s))) == [(3, 3), (8, 8)]


def test_suppression_is_strict():
    s = np.zeros((9, 9), np.uint8)
    s[4, 3] = s[4, 4] = 40                      # two adjacent equal corners both vanish
    assert not om.suppress(s).any()
    s[4, 4] = 41                                # of two unequal ones the larger stays
    assert list(zip(*np.nonzero(om.suppress(s)))) == [(4, 4)]
    s[5, 5] = 41                                # a diagonal neighbour counts
    assert not om.suppress(s).any()
    # the same through images: adjacent bright pixels lie off each other's ring, so both are corners
    e = dict(nfeatures=10, nlevels=1, edge_threshold=8, fast_threshold=20)
    d = om.detect(dots(40, 40, [(20, 20, 200), (21, 20, 200)]), **e)
    assert d.scores[0][20, 20] == d.scores[0][20, 21] == 149 and len(d.xy) == 0
    d = om.detect(dots(40, 40, [(20, 20, 200), (21, 20, 180)]), **e)
    assert d.scores[0][20, 21] == 129 and d.xy.tolist() == [[20.0, 20.0]]


def test_level_sizes_round_half_to_even():
    assert [om.level_size(163, 121, l) for l in range(3)] == [(163, 121), (82, 60), (41, 30)]
    assert [om.level_size(640, 480, l) for l in range(5)] == [(640, 480), (320, 240), (160, 120), (80, 60), (40, 30)]
    levels = om.build_levels(texture(163, 121), 3)
    assert [l.shape for l in levels] == [(121, 163), (60, 82), (30, 41)]


def test_resize_at_even_sizes_is_the_rounded_mean_of_2_x_2():
    img = np.random.default_rng(3).integers(0, 256, (48, 64)).astype(np.uint8)
    levels = om.build_levels(img, 3)
    for l in (1, 2):
        p = levels[l - 1].astype(np.int64)
        assert np.array_equal(levels[l], (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2)


def test_mask_levels():
    m = np.full((16, 16), 255, np.uint8)
    m[5, 8] = 0
    levels = om.build_mask_levels(m, 3)
    assert levels[1][2, 4] == 0 and np.count_nonzero(levels[1] == 0) == 1      # one zero among the four sources masks the pixel
    assert levels[2][1, 2] == 0 and np.count_nonzero(levels[2] == 0) == 1
    assert set(np.unique(levels[1])) == {0, 255}
    ones = om.build_mask_levels(np.ones((16, 16), np.uint8), 2)                # value 1: valid at level 0, masked above
    assert ones[0].all() and not ones[1].any()
    # through detect: a dot on a value-1 mask is found at level 0; the same dot under a zero byte is not
    img = dots(40, 40, [(20, 20, 200)])
    e = dict(nfeatures=10, nlevels=1, edge_threshold=8, fast_threshold=20)
    assert len(om.detect(img, np.ones((40, 40), np.uint8), **e).xy) == 1
    zero = np.full((40, 40), 255, np.uint8)
    zero[20, 20] = 0
    assert len(om.detect(img, zero, **e).xy) == 0
    # a masked corner still takes part in the suppression: its weaker neighbour does not appear in its place
    assert len(om.detect(dots(40, 40, [(20, 20, 200), (21, 20, 180)]), zero, **e).xy) == 0


def test_features_per_level_table():
    assert om.features_per_level(500, 5) == [258, 129, 65, 32, 16]
    assert om.features_per_level(1, 5) == [1, 0, 0, 0, 0]
    assert om.features_per_level(0, 5) == [0, 0, 0, 0, 0]
    assert om.features_per_level(500, 1) == [500]
    assert len(om.detect(texture(64, 64), nfeatures=0, nlevels=2, edge_threshold=8).xy) == 0


def test_features_per_level_of_the_library_equals_the_model():
    from dsopp_amd import capi
    for nlevels in range(1, 9):
        for nfeatures in range(0, 2001):
            assert capi.orb_features_per_level(nfeatures, nlevels).tolist() == om.features_per_level(nfeatures, nlevels), (nfeatures, nlevels)
    for bad in ((-1, 5), (10, 0), (10, 9)):
        with pytest.raises(capi.HipError):
            capi.orb_features_per_level(*bad)


def test_harris_on_a_ramp_and_on_a_dot():
    s4 = om.harris_scale4()
    assert s4 == ((F(1) / F(7140)) * (F(1) / F(7140))) * (F(1) / F(7140)) * (F(1) / F(7140))
    for g in (1, 3, 7):
        img = (g * np.arange(32))[None, :].repeat(20, axis=0).astype(np.uint8)
        assert om.harris_sums(img, 12, 10) == (49 * 64 * g * g, 0, 0)
        fa = F(49 * 64 * g * g)
        want = ((fa * F(0) - F(0) * F(0)) - (F(0.04) * (fa + F(0))) * (fa + F(0))) * s4
        got = om.harris_response(img, 12, 10)
        assert got.dtype == np.float32 and got == want and got < 0
        assert om.harris_sums(np.ascontiguousarray(img.T), 10, 12) == (0, 49 * 64 * g * g, 0)
    a, b, c = om.harris_sums(dots(30, 30, [(15, 15, 200)]), 15, 15)
    assert a == b > 0 and c == 0
    # the sums round once on their way to float32: 2^24 + 1 is not representable
    assert om.harris_from_sums(2 ** 24 + 1, 1, 0) == om.harris_from_sums(2 ** 24, 1, 0)


E1 = dict(nlevels=1, edge_threshold=8, fast_threshold=20)


def tie_dots(values):
    """dots of the given values 12 pixels apart on a row: the 9 x 9 neighbourhoods do not meet, equal values give equal responses"""
    return dots(16 + 12 * len(values), 32, [(12 + 12 * i, 16, v) for i, v in enumerate(values)])


def test_first_cut_keeps_the_whole_group_tied_at_its_boundary():
    values = [170, 140, 160, 140, 120, 140, 150]            # scores value - 51; 2 n = 4: the 4th largest is 140's, three of them
    d = om.detect(tie_dots(values), nfeatures=2, **E1)
    assert len(d.filtered[0][0]) == 7
    assert sorted(d.first_cut[0][2].tolist()) == sorted(v - BACKGROUND - 1 for v in values if v >= 140)
    assert d.xy.tolist() == [[12.0, 16.0], [36.0, 16.0]]    # then the two strongest responses, in canonical order
    # at most 2 n survivors: nothing is cut, whatever the scores
    assert len(om.detect(tie_dots(values[:4]), nfeatures=2, **E1).first_cut[0][0]) == 4


def test_second_cut_keeps_the_whole_group_of_equal_responses():
    values = [150, 180, 150, 110, 150]                      # first cut: 5 > 4, the 4th largest is 150's: 180 and three 150s stay
    d = om.detect(tie_dots(values), nfeatures=2, **E1)
    assert len(d.first_cut[0][0]) == 4
    r = d.response
    assert len(r) == 4 and r[1] > r[0] and r[0] == r[2] == r[3]         # an exact float tie at the boundary, kept whole
    assert d.xy[:, 0].tolist() == [12.0, 24.0, 36.0, 60.0]
    assert om.retain_best(np.array([1.0, -0.0, 0.0, -1.0], np.float32), 2).tolist() == [0, 1, 2]   # -0 equals +0
    assert om.retain_best(np.array([3, 1, 2]), 0).tolist() == [] and om.retain_best(np.array([3, 1, 2]), 3).tolist() == [0, 1, 2]


def test_shifting_a_texture_shifts_the_interior_detections_of_every_level():
    w, h, e, shift = 160, 120, 8, 16
    big = texture(w, h, margin=shift)
    a, b = big[shift:, shift:], big[:h, :w]                 # b[y + 16][x + 16] = a[y][x]
    kw = dict(nfeatures=100000, nlevels=3, edge_threshold=e, fast_threshold=20)   # no cut bites: each detection stands alone
    da, db = om.detect(a, **kw), om.detect(b, **kw)
    for l in range(3):
        s = shift >> l
        wl, hl = om.level_size(w, h, l)
        xa, ya, ra = da.final[l]
        xb, yb, rb = db.final[l]
        moved = {(x + s, y + s, r.tobytes()) for x, y, r in zip(xa, ya, ra) if x + s < wl - e and y + s < hl - e}
        inner = {(x, y, r.tobytes()) for x, y, r in zip(xb, yb, rb) if x - s >= e and y - s >= e}
        assert moved == inner and len(inner) > 5, (l, len(moved), len(inner))


def test_output_is_in_canonical_order_on_the_level_grids():
    d = om.detect(texture(160, 120), nfeatures=60, nlevels=3, edge_threshold=8)
    assert len(d.xy) >= 60 and set(d.level.tolist()) == {0, 1, 2}
    key = [(int(l), float(y), float(x)) for (x, y), l in zip(d.xy, d.level)]
    assert key == sorted(key) and len(set(key)) == len(key)
    for (x, y), l in zip(d.xy, d.level):
        assert x % (1 << l) == 0 and y % (1 << l) == 0
    assert d.xy.dtype == np.float32 and d.level.dtype == np.int32 and d.response.dtype == np.float32


def test_find_correspondences_first_frame_and_refill():
    from dsopp_amd import capi
    import optical_flow_model as ofm
    first = texture(96, 64, seed=5)
    new = om.detect(first, nfeatures=30, nlevels=2, edge_threshold=8).xy
    features, corr = om.find_correspondences(None, None, first, new, 30, capi.features_shuffle_order)
    assert np.array_equal(features, new) and corr.shape == (0, 2)
    tracker = ofm.Tracker(96, 64)
    tracker.set_reference(first)
    lost = np.array([[-40.0, -40.0], [500.0, 10.0]], np.float32)          # two features the flow cannot keep
    features_from = np.concatenate([new[:10], lost, new[10:20]])
    features, corr = om.find_correspondences(features_from, tracker, first, new, 22, capi.features_shuffle_order)
    assert corr[:, 0].tolist() == [i for i in range(22) if i not in (10, 11)] and corr[:, 1].tolist() == list(range(20))
    order = capi.features_shuffle_order(len(new))
    assert len(features) == 22 and np.array_equal(features[20:], new[order[:2]])


def build_example(tmp_path):
    libdir = os.path.join(ROOT, "dsopp_amd", "lib")
    exe = str(tmp_path / "example_find_correspondences")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "dsopp_amd", "host", "example_find_correspondences.cpp"),
                           f"-L{libdir}", "-ldsopp_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", exe])
    return exe


def test_example_driver_compiles_and_fails_loudly_without_gpu(tmp_path):
    from dsopp_amd import capi
    exe = build_example(tmp_path)
    if capi.device_count() == 0:                # (with a device tests/test_gpu_orb_detector.py runs it)
        r = subprocess.run([exe, "/nonexistent"], capture_output=True, text=True)
        assert r.returncode == 2 and "no CPU fallback" in r.stdout


def test_no_cpu_fallback():
    from dsopp_amd import capi
    if capi.device_count() == 0:
        with pytest.raises(capi.HipError) as e:
            capi.OrbDetector(64, 48)
        assert "no HIP device" in str(e.value) or "-4" in str(e.value)
    with pytest.raises(capi.HipError) as e:     # the arguments are judged first, with or without a device
        capi.OrbDetector(64, 48, nlevels=9)
    assert "-1" in str(e.value)
