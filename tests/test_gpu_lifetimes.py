"""Lifetimes of the library's handles: every kind is created, used and destroyed many times in a row, each time with device work
still queued or just finished, the way a long tracker run does.  Every call has to succeed, and a fresh handle of the same kind has
to work afterwards.  Run under `rocprofv3 --hip-trace --stats`, the balance of stream, event, pinned and device allocations against
their releases must not grow with DSOPP_LIFETIME_REPEATS (default 50)."""
import functools
import os

import numpy as np
import pytest

from dsopp_amd import synthetic as syn

pytestmark = pytest.mark.gpu

REPEATS = int(os.environ.get("DSOPP_LIFETIME_REPEATS", "50"))
W, H = 160, 120


@functools.lru_cache(maxsize=None)
def _window():
    return syn.make_window(num_frames=3, num_points=150, width=W, height=H, seed=1)


def _loaded_window(capi):
    g = capi.HipWindow(capi.default_pba_options())
    syn.load_window(g, _window())
    return g


def _pyramid(capi, frame):
    p = capi.Pyramid(W, H, 1)
    p.build(frame.image_u8)
    return p


def test_profiled_window_destroyed_with_its_timings_unread():
    from dsopp_amd import capi
    for _ in range(REPEATS):
        g = _loaded_window(capi)
        g.set_profiling(True)
        g.solve()
        g.close()   # the timing events of the solve were never collected
    g = _loaded_window(capi)
    g.set_profiling(True)
    g.solve()
    assert sum(n for _, n in g.get_profile().values()) > 0
    g.close()


def test_depth_maps_outlive_their_window_or_go_first():
    from dsopp_amd import capi
    intr = _window().scene.intrinsics
    T = syn.mat_to_params(np.eye(4))
    for k in range(REPEATS + 1):
        g = _loaded_window(capi)
        g.solve()
        maps = g.create_reference_depth_maps(1)
        flow = maps.mean_square_optical_flow(0, intr, [T])
        assert np.isfinite(flow).all()
        if k % 2:
            g.close()
            maps.get_level(0)   # on the device's default stream now
            maps.close()
        else:
            maps.close()
            g.close()


def test_immature_sets_destroyed_after_a_batched_estimate():
    from dsopp_amd import capi
    win = _window()
    intr = win.scene.intrinsics
    f0 = win.frames[0]
    n_sets = 9   # more than the launch arguments hold: the pinned descriptor tables of the lead set are used
    rng = np.random.default_rng(3)
    uv = np.stack([rng.integers(10, W - 10, 40), rng.integers(10, H - 10, 40)], axis=1).astype(np.float64)
    direction = np.stack([(uv[:, 0] - intr[2]) / intr[0], (uv[:, 1] - intr[3]) / intr[1], np.ones(len(uv))], axis=1)
    ui, vi = uv[:, 0].astype(int), uv[:, 1].astype(int)
    patch = np.stack([f0.pixelinfo[vi + int(oy), ui + int(ox), 0] for ox, oy in syn.PATTERN], axis=1)
    grad = np.stack([f0.pixelinfo[vi, ui, 1], f0.pixelinfo[vi, ui, 2]], axis=1)
    lms = syn.new_immature_landmarks(uv, direction, patch, grad)
    T_tr = syn.mat_to_params(np.linalg.inv(win.frames[1].T_w_c_gt) @ f0.T_w_c_gt)
    target = _pyramid(capi, win.frames[1])
    for _ in range(REPEATS + 1):
        sets = [capi.ImmatureSet(lms) for _ in range(n_sets)]
        capi.estimate_depths_batched(sets, target, 0, intr, np.tile(T_tr, (n_sets, 1)), np.ones(n_sets), np.zeros((n_sets, 2)))
        state = sets[0].download()
        assert (state["status"] != syn.IMMATURE_STATUS["uninitialized"]).any()
        for s in sets:
            s.close()
    target.close()


def test_aligner_destroyed_after_an_estimate():
    from dsopp_amd import capi
    win = _window()
    intr = win.scene.intrinsics
    ref, tgt = win.frames[-1], win.frames[-2]
    g = _loaded_window(capi)
    g.solve()
    maps = g.create_reference_depth_maps(1)
    T_ref, ab_ref = g.get_pose(ref.frame_id)
    ref_pyr, tgt_pyr = _pyramid(capi, ref), _pyramid(capi, tgt)
    for _ in range(REPEATS + 1):
        a = capi.HipAligner(capi.default_align_options())
        res = a.estimate_pose(ref.timestamp, T_ref, ref_pyr, maps, 1.0, ab_ref, tgt.timestamp + 1, tgt_pyr, 1.0, intr,
                              syn.mat_to_params(tgt.T_w_c_gt)[None], np.zeros(2), np.full(1, 1e10))
        assert np.isfinite(res["T_w_target"]).all()
        a.close()
    maps.close()
    g.close()
    ref_pyr.close()
    tgt_pyr.close()


def test_feature_extractor_destroyed_after_an_extraction():
    from dsopp_amd import capi
    img = _window().frames[0].image_u8
    found = None
    for _ in range(REPEATS + 1):
        ex = capi.FeatureExtractor(W, H)
        got = ex.extract(img)
        assert found is None or np.array_equal(got, found)   # a fresh extractor starts from the same state
        found = got
        ex.close()
    assert len(found) > 0


def test_pyramid_destroyed_after_set_and_get_level():
    from dsopp_amd import capi
    f0 = _window().frames[0]
    for _ in range(REPEATS + 1):
        p = capi.Pyramid(W, H, 1)
        p.build(f0.image_u8)
        p.set_level(0, f0.pixelinfo)
        assert np.array_equal(p.get_level(0), f0.pixelinfo)
        p.close()
