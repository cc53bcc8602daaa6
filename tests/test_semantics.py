"""The NumPy model of the semantic segmentation path (tests/semantics_model.py) on cases worked out by hand, the condition the GPU
observation tests rely on (no reprojection of the small_window scene lies within 1e-9 of a decision), and the presence of the
wrappers.  No GPU."""
import numpy as np

import semantics_model as sm

F = 7  # the filtered class of the hand-made case


def _hand_case():
    """8 x 8.  Valid pixels of level 0 (m0 != 0):
         block A (rows 0-3, cols 0-3): only (0, 0) — outside the block's centre 2 x 2; the rest is class 7
         block B (rows 0-3, cols 4-7): everything
         block C (rows 4-7, cols 0-3): everything but (5, 1) and (6, 1), which the static mask removes
         block D (rows 4-7, cols 4-7): only (5, 5), where the static mask holds the value 1; the rest is class 7"""
    static = np.full((8, 8), 255, dtype=np.uint8)
    static[5, 1] = static[6, 1] = 0
    static[5, 5] = 1
    cls = np.full((8, 8), 2, dtype=np.uint8)
    cls[0:4, 0:4] = F
    cls[0, 0] = 3
    cls[4:8, 4:8] = F
    cls[5, 5] = 0
    is_filtered = np.zeros(256, dtype=np.uint8)
    is_filtered[F] = 1
    return static, cls, is_filtered


def test_filter_and_mask_pyramid_by_hand():
    static, cls, is_filtered = _hand_case()
    m0 = sm.filter_mask(static, cls, is_filtered)
    expect0 = np.array([[255, 0, 0, 0, 255, 255, 255, 255],
                        [0, 0, 0, 0, 255, 255, 255, 255],
                        [0, 0, 0, 0, 255, 255, 255, 255],
                        [0, 0, 0, 0, 255, 255, 255, 255],
                        [255, 255, 255, 255, 0, 0, 0, 0],
                        [255, 0, 255, 255, 0, 1, 0, 0],
                        [255, 0, 255, 255, 0, 0, 0, 0],
                        [255, 255, 255, 255, 0, 0, 0, 0]], dtype=np.uint8)
    assert np.array_equal(m0, expect0)
    # level 1: (sum of the 2 x 2 block + 2) >> 2; one pixel of 255 gives 64, three give 191, the lone 1 of block D rounds to 0
    assert np.array_equal(sm.mask_level(m0, 1), np.array([[64, 0, 255, 255], [0, 0, 255, 255], [191, 255, 0, 0], [191, 255, 0, 0]], dtype=np.uint8))
    # level 2 reads rows 4y + 1 .. 4y + 2, cols 4x + 1 .. 4x + 2 of LEVEL 0: block A's only valid pixel is not among them, so it
    # reads 0, where the mean of level 1's block — (64 + 0 + 0 + 0 + 2) >> 2 = 16 — would have kept the texel valid
    assert np.array_equal(sm.mask_level(m0, 2), np.array([[0, 255], [128, 0]], dtype=np.uint8))
    chained = (sm.mask_level(m0, 1).astype(int)[0:2, 0:2].sum() + 2) >> 2
    assert chained == 16
    # level 3 reads rows 3-4, cols 3-4: 0, 255, 255, 0
    assert np.array_equal(sm.mask_level(m0, 3), np.array([[128]], dtype=np.uint8))
    valid, kept = sm.mask_pyramid(static, cls, is_filtered, 4)
    assert np.array_equal(kept, expect0)
    assert np.array_equal(valid[0], (expect0 != 0).astype(np.uint8))
    assert np.array_equal(valid[1], np.array([[1, 0, 1, 1], [0, 0, 1, 1], [1, 1, 0, 0], [1, 1, 0, 0]], dtype=np.uint8))
    assert np.array_equal(valid[2], np.array([[0, 1], [1, 0]], dtype=np.uint8))
    assert np.array_equal(valid[3], np.array([[1]], dtype=np.uint8))


def test_without_filter_or_class_image_the_static_mask_is_copied():
    static, cls, is_filtered = _hand_case()
    assert np.array_equal(sm.filter_mask(static, cls, None), static)
    assert np.array_equal(sm.filter_mask(static, None, is_filtered), static)
    valid, _ = sm.mask_pyramid(static, None, is_filtered, 2)
    assert valid[0].sum() == 62 and np.array_equal(valid[1], np.ones((4, 4), dtype=np.uint8))


def test_type_rule():
    counts = np.zeros(256, dtype=np.uint8)
    assert sm.semantic_type(counts) == 0 and sm.semantic_type(counts, sm.default_legend_weights()) == 0
    counts[[9, 4, 200]] = 5
    counts[17] = 3
    assert sm.semantic_type(counts) == 4                      # ties resolve to the first index
    w = np.zeros(256, dtype=np.uint64)
    assert sm.semantic_type(counts, w) == 4                   # every product 0: the first maximal count
    w[17], w[9], w[200] = 2, 1, 1
    assert sm.semantic_type(counts, w) == 17                  # 3 * 2 = 6 beats 5 * 1
    w[17] = 1
    assert sm.semantic_type(counts, w) == 9                   # 5 = 5: the first index with the strictly largest product
    # the legend quirk: weights_ = {1}, so a legend that lists nothing weighs code 0 alone
    assert sm.semantic_type(counts, sm.default_legend_weights()) == 4    # count[0] = 0: all products 0
    counts[0] = 1
    assert sm.semantic_type(counts, sm.default_legend_weights()) == 0    # one observation of code 0 outweighs five of any other
    assert np.array_equal(sm.semantic_types(np.stack([counts, np.zeros(256, dtype=np.uint8)]), None), [4, 0])


def _one_pair_scene(cls_value, repeats):
    """two frames at the same pose: every pattern point of a landmark at (20, 20) lands on itself in the other frame"""
    frames = {k: dict(T=np.eye(4), intr=(128.0, 128.0, 32.0, 24.0), width=64, height=48, uv=np.array([[20.0, 20.0]]), idepth=np.array([0.2]),
                      cls=np.full((48, 64), cls_value, dtype=np.uint8), marginalized=False) for k in (0, 1)}
    statuses = {(0, 1): np.zeros(1, dtype=np.uint8), (1, 0): np.zeros(1, dtype=np.uint8)}
    hist = None
    for _ in range(repeats):
        hist, pairs, near = sm.add_observations(frames, statuses, [0], hist)
    return hist, pairs, near


def test_counter_wraps_at_256():
    hist, pairs, _ = _one_pair_scene(5, 31)
    assert hist[0][0, 5] == 248 and hist[1][0, 5] == 248 and pairs[0][0] == 1
    hist, _, _ = _one_pair_scene(5, 32)
    assert hist[0][0, 5] == 0 and hist[0].sum() == 0            # 32 * 8 = 256 wraps to 0
    hist, _, _ = _one_pair_scene(5, 33)
    assert hist[0][0, 5] == 8 and hist[1][0, 5] == 8


def test_observation_rules():
    """truncated coordinates pick the class; statuses other than kOk, targets without a class image, frames flagged marginalised and
    pairs of two listed frames are skipped"""
    cls = np.zeros((48, 64), dtype=np.uint8)
    cls[:, 21:] = 9                                            # pattern points (21, 21), (22, 20) of a landmark at (20, 20)
    mk = lambda c, marg=False: dict(T=np.eye(4), intr=(128.0, 128.0, 32.0, 24.0), width=64, height=48, uv=np.array([[20.0, 20.0], [30.0, 30.0]]),  # noqa: E731
                                    idepth=np.array([0.2, 0.2]), cls=c, marginalized=marg)
    frames = {0: mk(cls), 1: mk(cls), 2: mk(None), 3: mk(cls, True)}
    statuses = {(r, t): np.array([0, 1], dtype=np.uint8) for r in frames for t in frames if r != t}
    hist, pairs, _ = sm.add_observations(frames, statuses, [0])
    assert hist[0][0, 9] == 2 and hist[0][0, 0] == 6           # from target 1 only: 2 has no class image, 3 is marginalised
    assert hist[0][1].sum() == 0                               # status 1 (outlier)
    assert hist[1][0, 9] == 2 and hist[2][0, 9] == 2           # frames 1 and 2 as references see frame 0's class image
    assert hist[3].sum() == 0 and pairs[3].sum() == 0
    hist, _, _ = sm.add_observations(frames, statuses, [0, 1])
    assert hist[0].sum() == 0 and hist[1].sum() == 0           # 0 and 1 pair only with each other (both listed) or with 2 (no class image)
    assert hist[2][0, 9] == 4                                  # reference 2 against both listed targets


def test_small_window_scene_has_no_near_ties(small_window):
    """the GPU tests leave out landmarks with a reprojection within 1e-9 of an integer or a ROI bound and bound their share by 1 %:
    with this scene and seed the model alone reports none"""
    win = small_window
    rng = np.random.default_rng(11)
    frames = {f.frame_id: dict(T=f.T_w_c_init, intr=win.scene.intrinsics, width=320, height=240, uv=f.uv, idepth=f.idepth_init,
                               cls=rng.integers(0, 6, (240, 320)).astype(np.uint8), marginalized=False) for f in win.frames}
    statuses = {(r.frame_id, t.frame_id): np.zeros(len(r.uv), dtype=np.uint8) for r in win.frames for t in win.frames if r is not t}
    hist, pairs, near = sm.add_observations(frames, statuses, [1])
    total, left_out = sum(int(p.sum()) for p in pairs.values()), sum(int(p[n > 0].sum()) for p, n in zip(pairs.values(), near.values()))
    assert total == 2 * 3 * 60 and left_out <= 0.01 * total
    assert sum(int(h.sum()) for h in hist.values()) > 8 * 0.5 * total   # most pairs reproject


def test_wrappers_exist():
    from dsopp_amd import capi
    for name in ("dsopp_hip_semantics_create", "dsopp_hip_semantics_destroy", "dsopp_hip_pyramid_set_semantics", "dsopp_hip_pyramid_get_semantics",
                 "dsopp_hip_pyramid_get_mask", "dsopp_hip_feature_extractor_set_mask_from_pyramid", "dsopp_hip_window_add_semantic_observations",
                 "dsopp_hip_window_get_semantic_observations", "dsopp_hip_window_get_semantic_types", "dsopp_hip_pyramid_group_set_semantics",
                 "dsopp_hip_window_group_add_semantic_observations", "dsopp_hip_window_group_get_semantic_observations",
                 "dsopp_hip_window_group_get_semantic_types"):
        assert name in capi.SYMBOLS, name
    assert callable(capi.Semantics) and callable(capi.Pyramid.set_semantics) and callable(capi.Pyramid.get_semantics) and callable(capi.Pyramid.get_mask)
    assert callable(capi.PyramidGroup.set_semantics) and callable(capi.FeatureExtractor.set_mask_from_pyramid)
    for cls in (capi.HipWindow, capi.HipWindowGroup):
        for method in ("add_semantic_observations", "get_semantic_observations", "get_semantic_types"):
            assert callable(getattr(cls, method)), (cls, method)
