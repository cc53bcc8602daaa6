"""tests/marginalization_model.py on cases worked by hand from the reference's strategy (sparse_frame_marginalization_strategy.cpp), and
the new entry points' declarations.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import marginalization_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dsopp_hip_window_note_optimization", "dsopp_hip_window_get_optimization_counts", "dsopp_hip_marginalization_default_options",
               "dsopp_hip_window_choose_marginalization"]


def frame(camera_id, t=(0.0, 0.0, 0.0), n=4, flags=None, n_inliers=5, successes=1, idepth=1.0, variance=1e-6, status="ok", immature=None):
    """a frame of n landmarks, all alike unless an array is given; status "ok": every landmark kOk in the last keyframe"""
    full = lambda v, dt: np.full(n, v, dtype=dt) if np.isscalar(v) else np.asarray(v, dtype=dt)  # noqa: E731
    return dict(camera_id=camera_id, t=np.asarray(t, np.float64), flags=np.zeros(n, np.uint8) if flags is None else np.asarray(flags, np.uint8),
                n_inliers=full(n_inliers, np.int32), successes=full(successes, np.int32), idepth=full(idepth, np.float64),
                variance=full(variance, np.float64), status_last=np.zeros(n, np.uint8) if isinstance(status, str) else status, immature=immature)


def line(A, **kw):
    """A frames one unit apart on the x axis, camera ids 10, 11, ..."""
    return [frame(10 + i, (float(i), 0.0, 0.0), **kw) for i in range(A)]


def untouched(frames, res):
    return all(np.array_equal(f["flags"], n) for f, n in zip(frames, res.flags))


@pytest.mark.parametrize("A", [0, 1, 2])
def test_at_most_two_active_frames_choose_nothing(A):
    # no status towards the last keyframe at all: the landmark rule would mark every landmark, it must not run
    frames = line(A, status=None, successes=0)
    res = mm.choose(frames)
    assert res.selected == [] and res.marginalized == [] and untouched(frames, res)
    assert res.n_newly_marginalized == 0 and res.n_newly_outlier == 0 and np.isnan(res.scores).all()


def test_window_that_fits_only_applies_the_landmark_rules():
    frames = line(7, successes=15)  # 7 > 7 is false: no score; 15 > 14 and 5 >= 3: valid for marginalisation
    frames[2]["successes"][1] = 14  # not more than 2 * maximum_size: stays
    frames[3]["n_inliers"][0] = 2   # fewer than (5 + 1) / 2: stays
    res = mm.choose(frames)
    assert res.selected == [] and res.marginalized == [] and np.isnan(res.scores).all()
    want = [np.full(4, 1, np.uint8) for _ in range(6)] + [np.zeros(4, np.uint8)]  # the last keyframe's landmarks are never looked at
    want[2][1] = 0
    want[3][0] = 0
    assert all(np.array_equal(a, b) for a, b in zip(res.flags, want))
    assert res.n_newly_marginalized == 22 and res.n_newly_outlier == 0


def test_all_frames_at_one_position_choose_index_zero():
    frames = [frame(10 + i) for i in range(8)]
    res = mm.choose(frames)
    # every distance is 0: score = sqrt(0) * 5 / 1e-5 = 0 for the six candidates, none exceeds max_score = 0, index 0 is inserted
    assert np.array_equal(res.scores[:6], np.zeros(6)) and np.isnan(res.scores[6:]).all()
    assert res.selected == [0] and res.marginalized == [0]
    assert np.array_equal(res.flags[0], np.full(4, 1, np.uint8))  # in the set: out of boundary, one success suffices
    assert all(np.array_equal(res.flags[a], np.zeros(4, np.uint8)) for a in range(1, 8))


def test_index_zero_is_chosen_when_every_candidate_is_too_young():
    frames = line(8)
    for f in frames:
        f["camera_id"] = 3  # id + kMinFrameAge > last id: every candidate is skipped
    res = mm.choose(frames)
    assert np.isnan(res.scores).all() and res.selected == [0] and res.marginalized == [0]


def test_score_by_hand():
    # candidates 0..6 of 9 frames; all at the last keyframe's position except frame 3, four units away:
    # score(3) = sqrt(4) * 6 / (1e-5 + 4), every other candidate sqrt(0) * ... = 0
    frames = [frame(10 + i) for i in range(9)]
    frames[3]["t"] = np.array([0.0, 4.0, 0.0])
    res = mm.choose(frames)
    want = np.zeros(7)
    want[3] = 2.0 * 6 / 4.00001
    assert np.allclose(res.scores[:7], want, rtol=1e-15, atol=0) and np.isnan(res.scores[7:]).all()
    assert res.selected == [3] and res.marginalized == [3]


def test_two_index_set_erases_a_shifted_frame():
    frames = [frame(10 + i) for i in range(9)]
    frames[3]["t"] = np.array([0.0, 4.0, 0.0])
    # frame 1: 100 landmarks, 96 of them marginalised: 4 < (1 - 0.95) * 100, and 9 - 0 > 5
    frames[1] = frame(11, n=100, flags=[1] * 96 + [0] * 4)
    res = mm.choose(frames)
    assert res.n_kept[1] == 4 and res.n_gone[1] == 96
    assert res.selected == [1, 3]  # 9 > 7 + 1: the score still runs and adds frame 3
    # erase(1) leaves [0, 2, 3, 4, ...]: erase(3) then hits frame 4, not frame 3
    assert res.marginalized == [1, 4]
    assert np.array_equal(res.flags[1], np.full(100, 1, np.uint8))
    assert np.array_equal(res.flags[3], np.full(4, 1, np.uint8))  # in the set: its landmarks go, the frame stays
    assert np.array_equal(res.flags[4], np.full(4, 1, np.uint8))  # not in the set: ActiveKeyframe::marginalize takes every landmark
    assert all(np.array_equal(res.flags[a], np.zeros(4, np.uint8)) for a in (0, 2, 5, 6, 7, 8))


def test_minimum_size_guard_stops_the_first_rule_mid_loop():
    gone = dict(n=20, flags=[2] * 20)  # nothing kept: 0 < 0.05 * 20
    frames = [frame(10 + i, **(gone if i < 4 else {})) for i in range(7)]
    res = mm.choose(frames)
    # i = 0: 7 - 0 > 5; i = 1: 7 - 1 > 5; i = 2: 7 - 2 > 5 is false, and stays false
    assert res.selected == [0, 1] and np.isnan(res.scores).all()  # 7 > 7 + 2 is false
    assert res.marginalized == [0, 2]  # the shifted erase again
    assert np.array_equal(res.flags[0], np.full(20, 3, np.uint8)) and np.array_equal(res.flags[2], np.full(20, 3, np.uint8))
    assert np.array_equal(res.flags[1], np.full(20, 2, np.uint8))  # outliers of a frame that stays are skipped
    assert res.n_newly_marginalized == 40 and res.n_newly_outlier == 0


def test_immature_landmarks_ready_for_activation_count_as_kept():
    imm = dict(status=np.array([0, 3, 4, 1, 2, 5, 6, 0, 0, 0], np.uint8), idepth_min=np.array([0.1] * 9 + [-1.0]), idepth_max=np.array([0.3] * 9 + [0.5]),
               uniqueness=np.array([4.0] * 7 + [3.0, 4.0, 4.0]), search_pixel_interval=np.array([1.0] * 8 + [8.0, 1.0]))
    assert np.array_equal(mm.ready_for_activation(imm), [1, 1, 1, 1, 0, 0, 0, 0, 0, 0])  # status, uniqueness > 3, interval < 8, idepth > 0
    f = frame(10, n=100, flags=[1] * 97 + [0] * 3, immature=imm)
    assert mm.counts(f) == (7, 97)
    frames = [f] + [frame(11 + i) for i in range(7)]
    assert mm.choose(frames).selected == [0]  # by the score (all zero), not by the first rule: 7 < 0.05 * 104 is false
    f["immature"] = None
    assert mm.counts(f) == (3, 97)


def test_landmark_rules():
    f = frame(10, n=6, successes=[0, 1, 15, 15, 0, 15], status=np.array([3, 3, 0, 0], np.uint8), idepth=[1, 1, 1, 1, 1, 1],
              variance=[1e-6, 1e-6, 1e-6, 1e-6, 1e-6, 1e-2])
    f["flags"][3] = 1
    frames = [f] + line(6)[1:]
    res = mm.choose(frames)
    # 0: out of boundary without a success: outlier.  1: out of boundary: marginalised.  2: kOk and valid: marginalised.  3: was marginalised.
    # 4, 5: no entry in the connection: not kOk — outlier, and marginalised with variance / idepth = 1e-2 > 1e-3: outlier as well
    assert np.array_equal(res.flags[0], [2, 1, 1, 1, 2, 3])
    f["status_last"] = None  # no connection at all
    assert np.array_equal(mm.choose(frames).flags[0], [2, 1, 1, 1, 2, 3])


def test_zero_and_negative_inverse_depth():
    assert mm.marginalize_landmark(0, 1e-6, 0.0) == 3   # 1e-6 / 0 = inf > 1e-3
    assert mm.marginalize_landmark(0, 0.0, 0.0) == 1    # 0 / 0 = NaN: neither comparison holds
    assert mm.marginalize_landmark(0, 1e-6, -1.0) == 3  # the quotient is negative, idepth < 0 marks it
    assert mm.marginalize_landmark(0, 1e-3, 1.0) == 1   # not strictly greater
    f = frame(10, n=4, idepth=[0.0, 0.0, -0.5, 2.0], variance=[1e-6, 0.0, 1e-6, 1e-6], status=np.full(4, 1, np.uint8))
    res = mm.choose([f] + line(3)[1:])
    assert np.array_equal(res.flags[0], [3, 1, 3, 1]) and res.n_newly_marginalized == 4 and res.n_newly_outlier == 2


def test_maximum_size_strategy():
    frames = line(9, n=3, status=None, successes=0)
    frames[1]["idepth"][2] = -1.0
    res = mm.choose(frames, mm.Options(strategy=mm.MAXIMUM_SIZE, maximum_size=7))
    assert res.selected == [0, 1] and res.marginalized == [0, 1] and np.isnan(res.scores).all()
    assert np.array_equal(res.flags[0], [1, 1, 1]) and np.array_equal(res.flags[1], [1, 1, 3])
    assert all(np.array_equal(res.flags[a], np.zeros(3, np.uint8)) for a in range(2, 9))  # no landmark rule in this strategy
    assert mm.choose(line(7), mm.Options(strategy=mm.MAXIMUM_SIZE, maximum_size=7)).marginalized == []


def test_counter():
    flags = np.array([0, 0, 1, 2, 3], np.uint8)
    n_inliers = np.array([4, 3, 9, 9, 9], np.int32)
    c = mm.note_optimization(np.zeros(5, np.int32), flags, n_inliers)
    assert np.array_equal(c, [1, 0, 0, 1, 0])  # more than 3 inliers, and not marginalised (an outlier still counts)
    assert np.array_equal(mm.note_optimization(c, flags, n_inliers), [2, 0, 0, 2, 0])


def test_erase_order():
    assert mm.erase_order([0, 1, 2], 8) == [0, 2, 4]
    assert mm.erase_order([5], 8) == [5]
    assert mm.erase_order([2, 3, 4, 5], 8) == [2, 4, 6]  # the fourth index is past the end of the five frames left


def test_header_declares_and_capi_lists_the_entry_points():
    from dsopp_amd import capi
    header = open(os.path.join(ROOT, "include", "dsopp_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b(int|void) %s\(" % name, header), name
        assert name in capi.SYMBOLS, name
    o = capi.MarginalizationOptions
    assert [n for n, _ in o._fields_] == ["strategy", "minimum_size", "maximum_size", "maximum_share_marginalized"]
    assert re.search(r"maximum_share_marginalized;\s*}\s*dsopp_hip_marginalization_options;", header)
    assert "HipFrameMarginalizationStrategy" in open(os.path.join(ROOT, "dsopp_amd", "host", "dsopp_hip_solvers.hpp")).read()


def test_default_options_are_the_reference_configuration():
    from dsopp_amd import capi
    o = capi.default_marginalization_options()
    assert (o.strategy, o.minimum_size, o.maximum_size, o.maximum_share_marginalized) == (capi.MARGINALIZATION_SPARSE, 5, 7, 0.95)
    assert mm.Options() == (mm.SPARSE, 5, 7, 0.95)


def build_example(tmp_path):
    libdir = os.path.join(ROOT, "dsopp_amd", "lib")
    exe = str(tmp_path / "example_marginalization")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "dsopp_amd", "host", "example_marginalization.cpp"),
                           f"-L{libdir}", "-ldsopp_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", exe])
    return exe


def test_example_driver_compiles_and_fails_loudly_without_gpu(tmp_path):
    from dsopp_amd import capi
    exe = build_example(tmp_path)
    if capi.device_count() > 0:
        pytest.skip("GPU present: tests/test_gpu_marginalization.py runs it")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "no CPU fallback" in r.stdout
