"""Semantic segmentation on the device against the NumPy model of tests/semantics_model.py: the per-frame masks of every pyramid
level and the kept class image (semantics.hip), their consumers, the extractor's mask taken from the pyramid, and the landmarks' class
observations in the window and the window group (semantic_observation_kernels.hpp).  The mask arithmetic is integer and the
observation counters are bytes: every comparison is bit for bit.  The one freedom is the last bit of a reprojected coordinate, which
the device forms from K [R | t] K^-1 and the model from rays: landmarks with a reprojection within 1e-9 of an integer or of a ROI bound
are left out, and the tests assert that they are at most 1 % of the (landmark, target) pairs (tests/test_semantics.py shows that the
scene has none)."""
import functools

import numpy as np
import pytest

import semantics_model as sm
import undistort_model as um
from dsopp_amd import synthetic as syn

pytestmark = pytest.mark.gpu

LEVELS = 4
N_CLASSES = 6
ERR_INVALID_ARGUMENT = -1
# 64 x 48: coarsest level 8 x 6; 200 x 136: odd coarse sizes (25 x 17) and several workgroups per level; 16 x 24: a 2 x 3 coarsest level
SIZES = {"64x48": (64, 48), "200x136": (200, 136), "16x24": (16, 24)}


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _class_image(W, H, seed):
    """piecewise constant over 6 classes: cells around 14 sites, their borders bent by a ripple"""
    rng = np.random.default_rng(seed)
    sites = np.stack([rng.uniform(0, W, 14), rng.uniform(0, H, 14)], axis=1)
    label = np.concatenate([np.arange(N_CLASSES), rng.integers(0, N_CLASSES, 14 - N_CLASSES)])
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    d = [(x - sx + 3 * np.sin(y / 3.1 + k)) ** 2 + (y - sy + 3 * np.cos(x / 2.7 + k)) ** 2 for k, (sx, sy) in enumerate(sites)]
    return _frozen(label[np.argmin(np.stack(d), axis=0)].astype(np.uint8))


@functools.lru_cache(maxsize=None)
def _static_mask(W, H):
    """a band, 15 % random zeros, and a few pixels of value 1 (an undistorted mask is not binary): alone in a block they round to 0"""
    rng = np.random.default_rng(W + 7 * H)
    m = np.full((H, W), 255, dtype=np.uint8)
    m[int(0.55 * H):int(0.55 * H) + 5, :] = 0
    r = rng.random((H, W))
    m[r < 0.15] = 0
    m[r > 0.97] = 1
    return _frozen(m)


@functools.lru_cache(maxsize=None)
def _is_filtered():
    f = np.zeros(256, dtype=np.uint8)
    f[[1, 4]] = (1, 200)   # any non-zero byte filters
    return _frozen(f)


@functools.lru_cache(maxsize=None)
def _image(W, H, seed):
    return _frozen(np.random.default_rng(seed).integers(0, 256, (H, W)).astype(np.uint8))


def _assert_masks(p, static, cls, is_filtered, what):
    valid, _ = sm.mask_pyramid(static, cls, is_filtered, LEVELS)
    for l in range(LEVELS):
        got = p.get_mask(l)
        assert got.shape == valid[l].shape and np.array_equal(got, valid[l]), (what, l, int((got != valid[l]).sum()))
    return valid


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("size", SIZES)
def test_masks_of_every_level_and_the_kept_class_image(size, dtype):
    from dsopp_amd import capi
    W, H = SIZES[size]
    static, filt = _static_mask(W, H), _is_filtered()
    cls_a, cls_b = _class_image(W, H, 1), _class_image(W, H, 2)
    all_valid = np.full((H, W), 255, dtype=np.uint8)
    on, no_filter, no_static = capi.Semantics(W, H, LEVELS, static, filt), capi.Semantics(W, H, LEVELS, static, None), capi.Semantics(W, H, LEVELS, None, filt)
    p = capi.Pyramid(W, H, LEVELS, capi.F64 if dtype == "f64" else capi.F32)
    try:
        # set_semantics BEFORE the first build: the build keeps the mask lane
        p.set_semantics(on, cls_a)
        p.build(_image(W, H, 5))
        valid = _assert_masks(p, static, cls_a, filt, "before build")
        assert all(0 < v.sum() < v.size for v in valid[:3])                 # the case is neither all valid nor all masked
        assert np.array_equal(p.get_semantics(), cls_a)
        texels = [p.get_level(l) for l in range(LEVELS)]
        # ... and AFTER it: another frame's class image, the texels' other lanes stay
        p.set_semantics(on, cls_b)
        other = _assert_masks(p, static, cls_b, filt, "after build")
        assert any(not np.array_equal(a, b) for a, b in zip(valid, other))  # the class image matters
        assert np.array_equal(p.get_semantics(), cls_b)
        assert all(np.array_equal(p.get_level(l), texels[l]) for l in range(LEVELS))
        # no filter: the static masks, the class image is still kept
        p.set_semantics(no_filter, cls_a)
        _assert_masks(p, static, None, None, "filter NULL")
        assert np.array_equal(p.get_semantics(), cls_a)
        # no class image for this frame
        p.set_semantics(on, None)
        _assert_masks(p, static, None, None, "class image NULL")
        assert p.get_semantics() is None
        # no static mask: all 255
        p.set_semantics(no_static, cls_a)
        _assert_masks(p, all_valid, cls_a, filt, "static NULL")
        # a rebuild keeps them
        p.build(_image(W, H, 6))
        _assert_masks(p, all_valid, cls_a, filt, "rebuild")
    finally:
        p.close()
        for s in (on, no_filter, no_static):
            s.close()


def _remap_maps(kind, in_size, out_size):
    (W, H), (w, h) = in_size, out_size
    if kind == "identity":
        return None, None
    if kind == "half_pixel":
        mx, my = um.identity_maps(w, h)
        return mx + np.float32(0.5), my + np.float32(0.5)
    mx, my = um.simple_radial_maps(w, h, 0.8 * w, 0.49 * w, 0.51 * h, -0.25, 0.06)
    stretch = lambda m, f: np.where(m == -1, m, m * np.float32(f)).astype(np.float32)  # noqa: E731
    return stretch(mx, W / w), stretch(my, H / h)


@pytest.mark.parametrize("kind,in_size", [("identity", (200, 136)), ("half_pixel", (200, 136)), ("simple_radial", (230, 150))])
def test_class_image_goes_through_the_undistorter(kind, in_size):
    """the class image is remapped by the camera's undistorter (bilinear over class codes, as the reference) before it filters"""
    from dsopp_amd import capi
    W, H = 200, 136
    mx, my = _remap_maps(kind, in_size, (W, H))
    static, filt = _static_mask(W, H), _is_filtered()
    distorted = _class_image(in_size[0], in_size[1], 3)
    cls = distorted.copy() if mx is None else um.remap(distorted, mx, my)
    u = capi.Undistorter(in_size, (W, H), mx, my)
    s = capi.Semantics(W, H, LEVELS, static, filt, undistorter=u)
    p = capi.Pyramid(W, H, LEVELS)
    try:
        p.build(_image(W, H, 5))
        p.set_semantics(s, distorted)
        assert np.array_equal(p.get_semantics(), cls)
        _assert_masks(p, static, cls, filt, kind)
        if kind != "identity":
            assert not np.array_equal(cls, distorted[:H, :W])
    finally:
        p.close()
        s.close()
        u.close()


def test_sizes_the_reference_cannot_mask_are_refused():
    """100 x 75 with 4 levels: already level 1 of the mask would have cvRound(37.5) = 38 rows against the image level's 75 >> 1 = 37"""
    from dsopp_amd import capi
    with pytest.raises(capi.HipError, match=f"error {ERR_INVALID_ARGUMENT}:"):
        capi.Semantics(100, 75, 4)
    with pytest.raises(capi.HipError, match=f"error {ERR_INVALID_ARGUMENT}:"):
        capi.Semantics(64, 48, 6)
    s = capi.Semantics(64, 48, 2)          # fewer levels than the pyramid
    t = capi.Semantics(128, 96, 4)         # another size
    p = capi.Pyramid(64, 48, 4)
    try:
        for bad in (s, t):
            with pytest.raises(capi.HipError, match=f"error {ERR_INVALID_ARGUMENT}:"):
                p.set_semantics(bad, None)
        assert all(p.get_mask(l).all() for l in range(4))   # untouched
    finally:
        p.close()
        s.close()
        t.close()


# ---- consumers ----------------------------------------------------------------------------------------------------------------------

def test_alignment_sees_the_semantic_masks():
    """one two-frame alignment per level against a target masked by set_semantics = the same against the model's masks uploaded by
    set_mask: every output equal"""
    from dsopp_amd import capi
    win = syn.make_window(num_frames=2, num_points=20, width=320, height=240, seed=7)
    fr, ft = win.frames
    H, W = fr.image_u8.shape
    static, filt, cls = _static_mask(W, H), _is_filtered(), _class_image(W, H, 4)
    valid, _ = sm.mask_pyramid(static, cls, filt, LEVELS)
    s = capi.Semantics(W, H, LEVELS, static, filt)
    pr, pa, pb, pc = (capi.Pyramid(W, H, LEVELS) for _ in range(4))
    try:
        pr.build(fr.image_u8)
        pa.build(ft.image_u8)
        pa.set_semantics(s, cls)
        pb.build(ft.image_u8)
        pc.build(ft.image_u8)           # the target without a mask
        for l in range(LEVELS):
            pb.set_mask(l, valid[l] * 255)
        rng = np.random.default_rng(5)
        T_ref, T_init = syn.mat_to_params(fr.T_w_c_gt), syn.mat_to_params(ft.T_w_c_init)
        for level in (0, 2):
            h, w = H >> level, W >> level
            intr = win.scene.intrinsics / (1 << level)
            n = 2500 >> level
            idsum, wgt = np.zeros((h, w)), np.zeros((h, w))
            xs, ys = rng.integers(0, w, n), rng.integers(0, h, n)
            idsum[ys, xs] = 1.0 / fr.depth[np.minimum(ys << level, H - 1), np.minimum(xs << level, W - 1)]
            wgt[ys, xs] = 1.0
            results = []
            for target in (pa, pb, pc):
                a = capi.HipAligner(capi.default_align_options())
                a.reset()
                a.push_reference_depth_map(1000, T_ref, pr, level, intr, idsum, wgt, 1.0, np.zeros(2))
                a.push_target(2000, T_init, target, level, intr, 1.0, np.zeros(2))
                results.append(a.solve())
                a.close()
            ra, rb, unmasked = results
            assert 0 < ra["n_valid"] < unmasked["n_valid"], level     # the mask matters
            assert set(ra) == set(rb)
            for k in ra:
                assert np.array_equal(np.asarray(ra[k]), np.asarray(rb[k])), (level, k)
    finally:
        for h_ in (pr, pa, pb, pc, s):
            h_.close()


def test_window_sweep_sees_the_semantic_masks(small_window):
    """one energy sweep of the window over pyramids masked by set_semantics = the same over the model's masks uploaded by set_mask"""
    from dsopp_amd import capi
    win = small_window
    W, H = 320, 240
    static, filt = _static_mask(W, H), _is_filtered()
    s = capi.Semantics(W, H, 1, static, filt)
    windows, keep = [], []
    try:
        for how in ("semantics", "set_mask", "none"):
            g = capi.HipWindow(capi.default_pba_options())
            g.set_deterministic(True)
            for i, f in enumerate(win.frames):
                p = capi.Pyramid(W, H, 1)
                keep.append(p)
                p.set_level(0, f.pixelinfo)
                cls = _class_image(W, H, 20 + i)
                if how == "semantics":
                    p.set_semantics(s, cls)
                elif how == "set_mask":
                    p.set_mask(0, sm.filter_mask(static, cls, filt))
                g.push_frame(f.frame_id, f.timestamp, None, None, win.scene.intrinsics, syn.mat_to_params(f.T_w_c_init), f.exposure, f.affine_init,
                             f.fixed, False, pyramid=p)
                g.set_landmarks(f.frame_id, f.uv, f.idepth_init, f.patch, np.zeros(len(f.uv), dtype=np.uint8))
                for j in range(i):
                    for (r, t) in ((win.frames[j], f), (f, win.frames[j])):
                        g.set_connection(r.frame_id, t.frame_id, np.zeros(len(r.uv), dtype=np.uint8))
            g.begin()
            windows.append((g, g.calculate_energy()))
        (ga, ea), (gb, eb), (_, e_none) = windows
        assert ea == eb and 0 < ea[1] < e_none[1]
        for fr in win.frames:
            for ft in win.frames:
                if fr is not ft:
                    ra, rb = ga.get_residuals(fr.frame_id, ft.frame_id), gb.get_residuals(fr.frame_id, ft.frame_id)
                    assert all(np.array_equal(ra[k], rb[k]) for k in ("status", "candidate", "energy")), (fr.frame_id, ft.frame_id)
    finally:
        for g, _ in windows:
            g.close()
        for p in keep:
            p.close()
        s.close()


@functools.lru_cache(maxsize=None)
def _textured_frame(W, H, i):
    T = syn.se3_exp(i * syn.BASE_MOTION)
    img, _ = syn.Scene.make(W, H, seed=11).render(T, 0.02 * i, 1.5 * i)
    return _frozen(np.clip(np.round(img), 0, 255).astype(np.uint8))


@pytest.mark.parametrize("kind", ["sobel", "eigen"])
def test_extractor_mask_from_pyramid(kind):
    """set_mask_from_pyramid + extract_from_pyramid = set_mask(the model's level-0 mask) + the same extract: lists and state, over
    two frames with different class images (the second call adapts the extractor's state)"""
    from dsopp_amd import capi
    W, H = 200, 136
    # (a band alone: the 15 x 15 erosion would leave nothing of a mask with 15 % random zeros)
    static, filt = np.full((H, W), 255, dtype=np.uint8), _is_filtered()
    static[int(0.55 * H):int(0.55 * H) + 5, :] = 0
    make = (lambda: capi.FeatureExtractor(W, H, 300.0)) if kind == "sobel" else (lambda: capi.EigenFeatureExtractor(W, H, 300.0))
    from_pyramid, from_host, unmasked = make(), make(), make()
    u = capi.Undistorter((W, H), (W, H))
    s = capi.Semantics(W, H, LEVELS, static, filt)
    p = capi.Pyramid(W, H, LEVELS)
    try:
        with pytest.raises(capi.HipError, match=f"error {ERR_INVALID_ARGUMENT}:"):
            from_pyramid.set_mask_from_pyramid(p)          # no set_semantics yet
        for i in range(2):
            cls = _class_image(W, H, 30 + i)
            p.build_undistorted(u, _textured_frame(W, H, i))
            p.set_semantics(s, cls)
            from_pyramid.set_mask_from_pyramid(p)
            got = from_pyramid.extract_from_pyramid(p, keep_mask=True)
            want = from_host.extract_from_pyramid(p, mask=sm.filter_mask(static, cls, filt))
            assert len(want) > 20 and got.shape == want.shape and np.array_equal(got, want), (kind, i, got.shape, want.shape)
            assert from_pyramid.state() == from_host.state(), (kind, i)
            if kind == "eigen":
                assert from_pyramid.stats() == from_host.stats(), i
            if i == 0:
                assert not np.array_equal(unmasked.extract_from_pyramid(p), want)   # the mask matters
    finally:
        for h_ in (from_pyramid, from_host, unmasked, p, s, u):
            h_.close()


# ---- class observations ---------------------------------------------------------------------------------------------------------------

W_OBS, H_OBS = 320, 240


def _frame_classes(win, without=()):
    return {f.frame_id: (None if f.frame_id in without else _class_image(W_OBS, H_OBS, 40 + f.frame_id)) for f in win.frames}


def _load(make_backend, win, classes, statuses=None, group=False, camera_masks=None):
    """the window (or group) with one single-level pyramid per frame that holds the frame's class image"""
    from dsopp_amd import capi
    g = make_backend()
    s = capi.Semantics(W_OBS, H_OBS, 1, None, None)
    keep = [s]
    for i, f in enumerate(win.frames):
        p = capi.PyramidGroup(g, W_OBS, H_OBS, 1) if group else capi.Pyramid(W_OBS, H_OBS, 1)
        keep.append(p)
        p.set_level(0, f.pixelinfo)
        p.set_semantics(s, classes[f.frame_id])
        if camera_masks is not None:
            p.set_mask(0, camera_masks[f.frame_id])
        g.push_frame(f.frame_id, f.timestamp, None, None, win.scene.intrinsics, syn.mat_to_params(f.T_w_c_init), f.exposure, f.affine_init, f.fixed,
                     False, pyramid=p)
        g.set_landmarks(f.frame_id, f.uv, f.idepth_init, f.patch, np.zeros(len(f.uv), dtype=np.uint8))
        for j in range(i):
            for (r, t) in ((win.frames[j], f), (f, win.frames[j])):
                st = None if statuses is None else statuses.get((r.frame_id, t.frame_id))
                g.set_connection(r.frame_id, t.frame_id, np.zeros(len(r.uv), dtype=np.uint8) if st is None else st)
    return g, keep


def _model_state(g, win, classes, marginalized=()):
    """the model's inputs read back from the window: current poses, inverse depths and connection statuses"""
    frames, statuses = {}, {}
    for f in win.frames:
        T, _ = g.get_pose(f.frame_id)
        frames[f.frame_id] = dict(T=syn.params_to_mat(T), intr=win.scene.intrinsics, width=W_OBS, height=H_OBS, uv=f.uv,
                                  idepth=g.get_landmarks(f.frame_id, False)["idepth"], cls=classes[f.frame_id], marginalized=f.frame_id in marginalized)
        for t in win.frames:
            if t is not f:
                statuses[(f.frame_id, t.frame_id)] = g.get_residuals(f.frame_id, t.frame_id)["status"]
    return frames, statuses


def _assert_histograms(g, win, want, pairs, near):
    total = sum(int(p.sum()) for p in pairs.values())
    left_out = sum(int(pairs[k][near[k] > 0].sum()) for k in pairs)
    assert total > 0 and left_out <= 0.01 * total, (left_out, total)
    for f in win.frames:
        got = g.get_semantic_observations(f.frame_id)
        sure = near[f.frame_id] == 0
        assert got.shape == want[f.frame_id].shape and np.array_equal(got[sure], want[f.frame_id][sure]), f.frame_id


def _window():
    from dsopp_amd import capi
    return capi.HipWindow(capi.default_pba_options())


@pytest.mark.parametrize("case", ["one_frame", "target_without_class_image", "two_frames_listed", "statuses", "partial_camera_mask", "after_solve"])
def test_class_observations(small_window, case):
    win = small_window
    rng = np.random.default_rng(17)
    classes = _frame_classes(win, without=(2,) if case == "target_without_class_image" else ())
    statuses = None
    if case == "statuses":   # a third of the entries are outlier / occluded / out of bounds
        statuses = {(r.frame_id, t.frame_id): rng.choice([0, 0, 0, 0, 1, 2, 3], len(r.uv)).astype(np.uint8) for r in win.frames for t in win.frames if r is not t}
    masks = None
    if case == "partial_camera_mask":   # the camera mask decides nothing here
        masks = {f.frame_id: (rng.random((H_OBS, W_OBS)) > 0.5).astype(np.uint8) * 255 for f in win.frames}
    listed = [1, 3] if case == "two_frames_listed" else [1]
    g, keep = _load(_window, win, classes, statuses, camera_masks=masks)
    try:
        if case == "after_solve":   # poses, inverse depths and statuses are then the solver's
            g.solve()
        assert all(not g.get_semantic_observations(f.frame_id).any() for f in win.frames)   # nothing counted yet
        for m in listed:
            g.mark_frame_marginalized(m)
        frames, sts = _model_state(g, win, classes)
        g.add_semantic_observations(listed)
        want, pairs, near = sm.add_observations(frames, sts, listed)
        _assert_histograms(g, win, want, pairs, near)
        counted = {k: int(h.any(axis=1).sum()) for k, h in want.items()}
        assert counted[1] > 30, counted
        if case == "two_frames_listed":
            assert counted[3] > 30 and all(counted[k] > 30 for k in (0, 2))
        if case == "statuses":
            assert any((s != 0).sum() > 10 for s in sts.values())
        # types, without a legend and with one
        weights = sm.default_legend_weights()
        weights[[1, 2, 3, 5]] = (3, 1, 40, 2)
        for f in win.frames:
            sure = near[f.frame_id] == 0
            for wt in (None, weights, np.zeros(256, dtype=np.uint64)):
                assert np.array_equal(g.get_semantic_types(f.frame_id, wt)[sure], sm.semantic_types(want[f.frame_id], wt)[sure]), (f.frame_id, wt is None)
        assert len(set(sm.semantic_types(want[1], weights))) > 2
        # a second add counts on; a frame marginalised EARLIER (flagged, not listed) takes no part
        if case == "one_frame":
            g.mark_frame_marginalized(2)
            frames, sts = _model_state(g, win, classes, marginalized=(2,))
            g.add_semantic_observations([1])
            want2, pairs2, near2 = sm.add_observations(frames, sts, [1], want)
            near2 = {k: near2[k] + near[k] for k in near}
            _assert_histograms(g, win, want2, pairs2, near2)
            assert np.array_equal(want2[2], want[2]) and not np.array_equal(want2[0], want[0])
    finally:
        g.close()
        for k in keep:
            k.close()


def test_counters_wrap_modulo_256(small_window):
    """a single-class image and 33 adds: every count is (33 * 8 * successful pairs) mod 256"""
    win = small_window
    classes = {f.frame_id: np.full((H_OBS, W_OBS), 5, dtype=np.uint8) for f in win.frames}
    g, keep = _load(_window, win, classes)
    try:
        g.mark_frame_marginalized(1)
        frames, sts = _model_state(g, win, classes)
        once, pairs, near = sm.add_observations(frames, sts, [1])
        for _ in range(33):
            g.add_semantic_observations([1])
        for f in win.frames:
            got, sure = g.get_semantic_observations(f.frame_id), near[f.frame_id] == 0
            successful = once[f.frame_id][:, 5].astype(np.int64) // 8
            assert np.array_equal(got[sure, 5], ((33 * 8 * successful) % 256).astype(np.uint8)[sure]), f.frame_id
            assert not np.delete(got, 5, axis=1).any()
        assert (once[1][:, 5] == 24).sum() > 10      # three successful pairs: 33 * 24 = 792 = 3 * 256 + 24 has wrapped three times
    finally:
        g.close()
        for k in keep:
            k.close()


def test_counters_survive_appended_landmarks(small_window):
    """set_landmarks appends to a keyframe that has counters (and re-orders nothing the counters depend on): the old rows stay, the
    new rows are zero, and the next add counts for both"""
    win = small_window
    classes = _frame_classes(win)
    first = {f.frame_id: 37 for f in win.frames}   # landmarks of the first batch
    from dsopp_amd import capi
    g = capi.HipWindow(capi.default_pba_options())
    s = capi.Semantics(W_OBS, H_OBS, 1)
    keep = [s]
    try:
        for i, f in enumerate(win.frames):
            p = capi.Pyramid(W_OBS, H_OBS, 1)
            keep.append(p)
            p.set_level(0, f.pixelinfo)
            p.set_semantics(s, classes[f.frame_id])
            n = first[f.frame_id]
            g.push_frame(f.frame_id, f.timestamp, None, None, win.scene.intrinsics, syn.mat_to_params(f.T_w_c_init), f.exposure, f.affine_init, f.fixed,
                         False, pyramid=p)
            g.set_landmarks(f.frame_id, f.uv[:n], f.idepth_init[:n], f.patch[:n], np.zeros(n, dtype=np.uint8))
            for j in range(i):
                for (r, t) in ((win.frames[j], f), (f, win.frames[j])):
                    g.set_connection(r.frame_id, t.frame_id, np.zeros(first[r.frame_id], dtype=np.uint8))
        g.mark_frame_marginalized(1)

        def model(n_of, hist):
            frames, sts = {}, {}
            for f in win.frames:
                n = n_of[f.frame_id]
                frames[f.frame_id] = dict(T=syn.params_to_mat(g.get_pose(f.frame_id)[0]), intr=win.scene.intrinsics, width=W_OBS, height=H_OBS, uv=f.uv[:n],
                                          idepth=f.idepth_init[:n], cls=classes[f.frame_id], marginalized=False)
                for t in win.frames:
                    if t is not f:
                        sts[(f.frame_id, t.frame_id)] = np.zeros(n, dtype=np.uint8)
            return sm.add_observations(frames, sts, [1], hist)

        g.add_semantic_observations([1])
        want, pairs, near = model(first, None)
        _assert_histograms(g, win, want, pairs, near)
        for f in win.frames:   # the rest of every keyframe's landmarks, connected to every other frame
            n = len(f.uv)
            g.set_landmarks(f.frame_id, f.uv, f.idepth_init, f.patch, np.zeros(n, dtype=np.uint8))
            for t in win.frames:
                if t is not f:
                    g.set_connection(f.frame_id, t.frame_id, np.zeros(n, dtype=np.uint8))
        grown = {k: np.concatenate([h, np.zeros((60 - len(h), 256), dtype=np.uint8)]) for k, h in want.items()}
        for f in win.frames:
            got = g.get_semantic_observations(f.frame_id)
            assert got.shape == (60, 256) and not got[37:].any()
            assert np.array_equal(got[:37][near[f.frame_id] == 0], want[f.frame_id][near[f.frame_id] == 0])
        g.add_semantic_observations([1])
        want2, pairs2, near2 = model({f.frame_id: 60 for f in win.frames}, grown)
        near2 = {k: near2[k] + np.concatenate([near[k], np.zeros(60 - 37, dtype=np.int64)]) for k in near2}
        _assert_histograms(g, win, want2, pairs2, near2)
        assert want2[1][37:].any()
    finally:
        g.close()
        for k in keep:
            k.close()


@pytest.mark.parametrize("shards", [1, 3])
def test_group_class_observations_match_the_single_window(small_window, shards):
    """every shard counts for its own landmarks (LOCAL transport, all shards on one device); the getters interleave"""
    from dsopp_amd import capi
    win = small_window
    rng = np.random.default_rng(23)
    classes = _frame_classes(win)
    statuses = {(r.frame_id, t.frame_id): rng.choice([0, 0, 0, 1, 3], len(r.uv)).astype(np.uint8) for r in win.frames for t in win.frames if r is not t}
    g1, keep1 = _load(_window, win, classes, statuses)
    gg, keep2 = _load(lambda: capi.HipWindowGroup(capi.default_pba_options(), devices=[0] * shards, transport=capi.TRANSPORT_LOCAL), win, classes, statuses,
                      group=True)
    try:
        weights = sm.default_legend_weights()
        weights[[1, 2, 3, 5]] = (3, 1, 40, 2)
        for w in (g1, gg):
            w.mark_frame_marginalized(1)
            w.add_semantic_observations([1])
            w.add_semantic_observations([1])
        frames, sts = _model_state(g1, win, classes)
        once, pairs, near = sm.add_observations(frames, sts, [1])
        want, _, _ = sm.add_observations(frames, sts, [1], once)
        _assert_histograms(g1, win, want, pairs, near)
        for f in win.frames:
            a, b = g1.get_semantic_observations(f.frame_id), gg.get_semantic_observations(f.frame_id)
            assert a.any() and np.array_equal(a, b), f.frame_id
            for wt in (None, weights):
                assert np.array_equal(g1.get_semantic_types(f.frame_id, wt), gg.get_semantic_types(f.frame_id, wt)), f.frame_id
    finally:
        g1.close()
        gg.close()
        for k in keep1 + keep2:
            k.close()
