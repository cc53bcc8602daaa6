"""The NumPy model of the eigen tracking-feature extractor (tests/eigen_features_model.py) pinned on hand-derived cases, its
order-free parallel formulation checked against the sequential walk, and the library's random pattern (dsopp_hip_eigen_random_pattern:
no device needed) against glibc's own rand().  What test_gpu_eigen_features.py holds the device to is only as good as this model."""
import ctypes
import ctypes.util

import numpy as np
import pytest

import eigen_features_model as em

ERR_INVALID_ARGUMENT = -1


def _glibc_pattern(n):
    libc = ctypes.CDLL(ctypes.util.find_library("c") or "libc.so.6")
    libc.srand(3141592)
    return np.array([libc.rand() & 0xFF for _ in range(n)], dtype=np.uint8)


@pytest.mark.parametrize("size", [(32, 32), (64, 33), (640, 480), (643, 481)])
def test_random_pattern_is_glibc_rand(size):
    from dsopp_amd import capi
    W, H = size
    want = _glibc_pattern(W * H)
    got = capi.eigen_random_pattern(W, H)
    assert got.shape == (H, W) and np.array_equal(got.ravel(), want)
    assert np.array_equal(em.random_pattern(W * H), want)


def test_random_pattern_and_create_refuse_bad_sizes():
    from dsopp_amd import capi
    out = np.zeros(4, dtype=np.uint8)
    for W, H in ((0, 4), (4, 0), (-1, 4)):
        assert capi.lib().dsopp_hip_eigen_random_pattern(W, H, out.ctypes.data_as(ctypes.c_void_p)) == ERR_INVALID_ARGUMENT
    h = ctypes.c_void_p()
    for W, H, d in ((31, 64, 100.0), (64, 31, 100.0), (64, 64, 0.0), (64, 64, float("nan"))):
        rc = capi.lib().dsopp_hip_feature_extractor_create_eigen(0, None, W, H, ctypes.c_double(d), ctypes.byref(h))
        assert rc == ERR_INVALID_ARGUMENT and not h.value, (W, H, d, rc)


DIRECTIONS_HEX = (
    ("0x1.9f05cb00a3700p-16", "-0x1.00003b6f489d7p+0"), ("0x1.8f8ef10a73c14p-3", "-0x1.f62998762549dp-1"),
    ("0x1.87de88aa6f384p-2", "-0x1.d906c20144f74p-1"), ("0x1.1c73bb3d82701p-1", "-0x1.a9b6633f8ef9cp-1"),
    ("0x1.6a09e73a60a73p-1", "-0x1.6a09e676fcbb2p-1"), ("0x1.a9b6629cc9d94p-1", "-0x1.1c73b39b89649p-1"),
    ("0x1.d906bcf35d9edp-1", "-0x1.87de2a6aee5b4p-2"), ("0x1.f6297cff75d84p-1", "-0x1.8f8b83c69a619p-3"),
    ("0x1.0000000000000p+0", "0x0.0p+0"), ("0x1.f6297cff75d84p-1", "0x1.8f8b83c69a619p-3"),
    ("0x1.d906bcf35d9edp-1", "0x1.87de2a6aee5b4p-2"), ("0x1.a9b6629cc9d95p-1", "0x1.1c73b39b89647p-1"),
    ("0x1.6a09e73a60a73p-1", "0x1.6a09e676fcbb2p-1"), ("0x1.1c73bb3d826ffp-1", "0x1.a9b6633f8ef9dp-1"),
    ("0x1.87de88aa6f384p-2", "0x1.d906c20144f74p-1"), ("0x1.8f8ef10a73c1cp-3", "0x1.f62998762549dp-1"),
)


def test_direction_table_is_pinned():
    """the Taylor polynomials as written, bit for bit: not cos / sin (i = 0 is not exactly (0, -1)), i = 8 exactly (1, 0)"""
    want = np.array([[float.fromhex(c), float.fromhex(s)] for c, s in DIRECTIONS_HEX])
    assert np.array_equal(em.DIRECTIONS, want)
    assert tuple(em.DIRECTIONS[8]) == (1.0, 0.0)
    assert em.DIRECTIONS[0, 0] != 0.0 and abs(em.DIRECTIONS[0, 1] + 1) > 1e-6
    assert np.abs(np.hypot(em.DIRECTIONS[:, 0], em.DIRECTIONS[:, 1]) - 1).max() < 1e-5


def test_median_bin_hand_histograms():
    h = np.zeros(50, dtype=np.int64)
    assert em._median_bin(h) == 0                 # empty: the sum never passes 0
    h[5] = 1
    assert em._median_bin(h) == 0                 # round(0.5) = 1: 1 - 1 = 0 is not below zero
    h[:] = 0
    h[3], h[7] = 1, 1
    assert em._median_bin(h) == 7
    h[:] = 0
    h[1], h[2], h[3] = 1, 1, 1
    assert em._median_bin(h) == 3                 # round(1.5) = 2


def test_threshold_map_empty_cell_and_clipped_mean():
    W = H = 64
    dx = np.full((H, W), 3.0)
    valid = np.ones((H, W), dtype=bool)
    valid[:32, :32] = False                       # cell (0, 0) has no valid pixel: median 0, raw 7
    tm = em.threshold_map(dx, np.zeros_like(dx), valid)
    assert tm.shape == (2, 2)
    assert np.all(tm == ((7 + 10 + 10 + 10) / 4.0) ** 2)   # every cell's clipped 3 x 3 is the whole 2 x 2 map


def test_threshold_map_three_by_three():
    W = H = 96
    dx = np.zeros((H, W))
    for j in range(3):
        for i in range(3):
            dx[32 * j:32 * (j + 1), 32 * i:32 * (i + 1)] = 1 + i + 3 * j   # raw = 8 + i + 3 j
    tm = em.threshold_map(dx, np.zeros_like(dx), np.ones((H, W), dtype=bool))
    assert tm[0, 0] == ((8 + 9 + 11 + 12) / 4.0) ** 2
    assert tm[1, 1] == 12.0 ** 2
    assert tm[0, 1] == ((8 + 9 + 10 + 11 + 12 + 13) / 6.0) ** 2
    assert tm[2, 2] == ((12 + 13 + 15 + 16) / 4.0) ** 2


def test_threshold_map_odd_size_excludes_the_frame():
    """70 x 45: 2 x 1 cells of 35 x 45; the histogram rows are [1, 43) and cell 1's columns [35, 68): the excluded pixels (dx 10)
    would move cell 1's median from 30 to 20"""
    W, H = 70, 45
    dx = np.full((H, W), 10.0)
    dx[:, :35] = 5.0
    dx[1:22, 35:68] = 20.0
    dx[22:43, 35:68] = 30.0
    tm = em.threshold_map(dx, np.zeros_like(dx), np.ones((H, W), dtype=bool))
    assert tm.shape == (1, 2)
    assert np.all(tm == ((12.0 + 37.0) / 2) ** 2)


def _fields(W, H, grads, tmap_value=49.0, valid=None):
    """hand-made fields: grads {(level, x, y): (dx, dy)} in level coordinates, every other gradient 0, a constant threshold map"""
    infos = [np.zeros((H >> l, W >> l, 3)) for l in range(em.LEVELS)]
    for (l, x, y), (gx, gy) in grads.items():
        infos[l][y, x, 1:] = (gx, gy)
    tmap = np.full((H // 32, W // 32), float(tmap_value))
    return em.Fields(infos, tmap, np.ones((H, W), dtype=bool) if valid is None else valid)


def _walks(F, p):
    """the literal walk, the fast walk and the parallel prototype give one list"""
    pattern = em.random_pattern(F.W * F.H)
    a = em.walk_literal(F, p, pattern)
    assert em.walk(F, p, pattern) == a
    assert em.ParallelPrototype(F, p, pattern).run()[0] == a
    return a


def test_pixel_border_is_inclusive_in_y_only():
    W = H = 64
    g = {(0, 10, 59): (10.0, 0.0), (0, 10, 60): (10.0, 0.0), (0, 59, 20): (10.0, 0.0), (0, 58, 20): (10.0, 0.0)}
    # y = H - 5 = 59 is inside, y = 60 is not; x = W - 5 = 59 is outside (x < W - 5); top windows in row-major order
    assert _walks(_fields(W, H, g), 1) == [(20 * W + 58, 0), (59 * W + 10, 0)]


def test_a_masked_corner_skips_the_whole_window():
    W = H = 64
    g = {(0, 13, 13): (10.0, 0.0)}
    want = [(13 * W + 13, 0)]
    assert _walks(_fields(W, H, g), 2) == want

    def masked(*pixels):
        v = np.ones((H, W), dtype=bool)
        for x, y in pixels:
            v[y, x] = False
        return v
    assert _walks(_fields(W, H, g, valid=masked((12, 12))), 2) == []    # the level-0 window's corner
    assert _walks(_fields(W, H, g, valid=masked((8, 8))), 2) == []      # the level-2 window's corner
    assert _walks(_fields(W, H, g, valid=masked((13, 12))), 2) == want  # a pixel of the window that is no corner
    assert _walks(_fields(W, H, g, valid=masked((13, 13))), 2) == []    # the pixel itself


def test_a_lower_level_blocks_the_levels_above():
    """p = 2: pixel (8, 8) is accepted on level 1, then (10, 8) on level 0 turns level 1 into -2: the level-1 window emits nothing,
    and (8, 10), which only level 1 would take, is skipped"""
    W = H = 64
    g = {(1, 4, 4): (10.0, 0.0), (0, 10, 8): (10.0, 0.0), (1, 4, 5): (10.0, 0.0)}
    assert _walks(_fields(W, H, g), 2) == [(8 * W + 10, 0)]
    del g[(0, 10, 8)]
    assert _walks(_fields(W, H, g), 2) == [(8 * W + 8, 1)]


def test_the_weight_is_the_squared_gradient():
    """one level-0 window (p = 4, corner (8, 8)), n = 0: a (dx 8) is accepted with weight 64; b (dx 30) and c (dx 100) project below
    64 and are not; d (dx 200) projects above it"""
    W = H = 64
    d = int(em.random_pattern(W * H)[0]) & 15
    c = em.DIRECTIONS[d, 0]
    assert d == 14 and 0.38 < c < 0.39
    g = {(0, 8, 8): (8.0, 0.0), (0, 9, 8): (30.0, 0.0), (0, 10, 8): (100.0, 0.0)}
    assert 30 * c < 100 * c < 64
    assert _walks(_fields(W, H, g), 4) == [(8 * W + 8, 0)]
    g[(0, 11, 8)] = (200.0, 0.0)
    assert 200 * c > 64
    assert _walks(_fields(W, H, g), 4) == [(8 * W + 11, 0)]
    del g[(0, 8, 8)]
    assert _walks(_fields(W, H, g), 4) == [(8 * W + 9, 0)]    # b (weight 900), then c and d fail: 100 c, 200 c < 900
    assert 200 * c < 900


def _fake(counts):
    """a walker that emits counts[p] features at distinct pixels"""
    def walker(F, p, pattern):
        return [((37 * k) % len(pattern), 0) for k in range(counts[p])]
    return walker


@pytest.mark.parametrize("density, counts, passes, potentials, kept_rule", [
    (1000.0, {15: 100, 4: 900}, 2, [15, 4], None),              # ratio 10: ideal (int)(sqrt(0.1) 16 - 1) = 4
    (100.0, {15: 1000, 49: 300}, 2, [15, 49], 85),              # ratio 0.1: ideal 49 > 16; then 1/3: reduced to pattern <= 85
    (100.0, {15: 90}, 1, [15, 0], None),                        # 1.11: one pass, no reduction
    (100.0, {15: 200}, 1, [15, 0], 127),                        # 0.5: one pass, reduced to pattern <= 127
    (10.0, {15: 0, 1: 0}, 2, [15, 1], None),                    # nothing found: ratio inf, ideal 1
    (100.0, {15: 1000, 49: 1000}, 2, [15, 49], 25),             # still below 0.25 after the second pass: no third
])
def test_potential_control(density, counts, passes, potentials, kept_rule):
    W, H = 64, 64
    m = em.EigenExtractorModel(W, H, density, walker=_fake(counts))
    xy = m.extract_fields(None)
    found = [counts[potentials[0]], counts[potentials[1]] if passes == 2 else 0]
    assert m.stats == dict(passes=passes, potentials=potentials, found=found)
    assert m.potential == potentials[passes - 1] and m.found_last == found[passes - 1]
    idx = [f for f, _ in _fake(counts)(None, potentials[passes - 1], m.pattern)]
    if kept_rule is not None:
        assert kept_rule == int(255.0 * (density / found[passes - 1]))
        idx = [i for i in idx if m.pattern[i] <= kept_rule]
    assert np.array_equal(xy, np.array([[i % W, i // W] for i in idx], dtype=np.float64).reshape(-1, 2))


def test_the_potential_persists_and_one_is_final():
    """the window size carries into the next call; at 1 a high ratio cannot shrink it further"""
    m = em.EigenExtractorModel(64, 64, 1000.0, walker=_fake({15: 100, 4: 100, 1: 10}))
    m.extract_fields(None)
    assert m.stats["potentials"] == [15, 4] and m.potential == 4       # ideal (int)(sqrt(0.1) 16 - 1) = 4
    m.extract_fields(None)
    assert m.stats["potentials"] == [4, 1] and m.potential == 1        # ideal (int)(sqrt(0.1) 5 - 1) = 0 -> 1
    m.extract_fields(None)
    assert m.stats == dict(passes=1, potentials=[1, 0], found=[10, 0]) and m.potential == 1


def smooth_ramp(W, H):
    ys, xs = np.mgrid[0:H, 0:W]
    return np.clip(np.round(20 + 0.2 * xs + 0.15 * ys), 0, 255).astype(np.uint8)


def test_smooth_ramp_emits_only_on_coarse_levels():
    W, H = 160, 128
    m = em.EigenExtractorModel(W, H, 7.0)
    F = m.fields(smooth_ramp(W, H))
    assert not F.A[0].any() and not F.A[1].any()           # level-0 / 1 gradients stay under their thresholds
    feats = _walks(F, 15)
    assert len(feats) > 0 and min(level for _, level in feats) >= 2


def _random_image(rng, kind, W, H):
    ys, xs = np.mgrid[0:H, 0:W]
    if kind == 0:     # constant rows: dx = 0 everywhere
        return np.repeat(np.clip(np.cumsum(rng.integers(-9, 10, H)) + 128, 0, 255)[:, None], W, axis=1).astype(np.uint8)
    if kind == 1:
        return rng.integers(0, 256, (H, W)).astype(np.uint8)
    if kind == 2:
        return np.clip(128 + 60 * np.sin(xs / 7.0) * np.cos(ys / 9.0) + rng.normal(0, 3, (H, W)), 0, 255).astype(np.uint8)
    return ((xs // int(rng.integers(3, 9)) + ys // int(rng.integers(3, 9))) % 2 * 90 + 60).astype(np.uint8)


def test_parallel_prototype_equals_the_sequential_walk():
    """52 random images of 64 x 64 to 160 x 128, p 1-6, random masks: the order-free counts of determined top windows equal their
    walks, and the assembled list (split top windows walked per level-2 window) equals the sequential one; constant-row images must
    have undetermined (chained) windows"""
    rng = np.random.default_rng(7)
    chained_const, split = [], 0
    for t in range(52):
        W, H = int(rng.integers(64, 161)), int(rng.integers(64, 129))
        p = int(rng.integers(1, 7)) if W * H < 12000 else int(rng.integers(2, 7))
        kind = t % 4
        img = _random_image(rng, kind, W, H)
        mask = None if t % 3 == 0 else (rng.random((H, W)) > 0.003).astype(np.uint8) * 255
        m = em.EigenExtractorModel(W, H, 100.0)
        F = m.fields(img, mask)
        seq = em.walk(F, p, m.pattern)
        proto = em.ParallelPrototype(F, p, m.pattern)
        par, chained, per_top = proto.run()
        assert par == seq, (t, W, H, p)
        split += proto.split
        for (E, determined), (x, y) in zip(per_top, em.top_windows(W, H, p)):
            if determined:
                assert E == len(em.walk_top(F, p, m.pattern, x, y, 0)), (t, x, y)
        if kind == 0:
            chained_const.append(chained)
        if t < 12:
            assert em.walk_literal(F, p, m.pattern) == seq, (t, W, H, p)
    assert min(chained_const) > 0
    assert split > 0   # top windows walked as 16 independent level-2 windows


HOST_SNIPPET = r"""
#include "dsopp_hip_solvers.hpp"
#include <cstdio>
using namespace dsopp_hip_host;
// both extractor kinds feed DeviceImmatureSet through the shared base
int main() {
  try {
    std::vector<uint8_t> image(64 * 48, 128);
    HipEigenTrackingFeaturesExtractor eigen(64, 48, 100.0);
    HipSobelTrackingFeaturesExtractor sobel(64, 48);
    DevicePyramid pyramid(64, 48, 1);
    const PinholeModel model{50, 50, 32, 24};
    std::vector<ImmatureLandmarkView> landmarks;
    const HipTrackingFeaturesExtractor *kinds[2] = {&eigen, &sobel};
    for (const HipTrackingFeaturesExtractor *ex : kinds) DeviceImmatureSet set(*ex, pyramid, model, landmarks);
    std::printf("%zu\n", eigen.extract(image.data(), nullptr).size());
  } catch (const SolverError &e) {
    std::printf("%s\n", e.what());
    return 2;
  }
  return 0;
}
"""


def test_host_mirror_offers_the_eigen_extractor(tmp_path):
    """HipEigenTrackingFeaturesExtractor and DeviceImmatureSet's constructor from either extractor compile with plain g++ -Werror and link
    against the C-ABI"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "dsopp_amd", "lib")
    src = tmp_path / "eigen_host.cpp"
    src.write_text(HOST_SNIPPET)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", f"-I{os.path.join(root, 'dsopp_amd', 'host')}", str(src),
                           f"-L{libdir}", "-ldsopp_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib",
                           "-o", str(tmp_path / "eigen_host")])
