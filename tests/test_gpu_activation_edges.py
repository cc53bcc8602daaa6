"""The HIP landmark activator (dsopp_hip_window_activate_landmarks: csrc/activation_kernels.hpp and its host set-up) against
tests/activation_model.py on the scenes of tests/activation_scenes.py: selection ties, dependency chains, neighbour-list overflow, the
greedy rounds' work-list boundary, grid-cell edges, mask rounding, the status table, count edges, more than 8 target keyframes and every
exit of the refinement.  tests/test_activation_model.py pins the model and the scenes on the CPU.

Two decisions of the kernels cannot be told apart by any output, so no scene here does: `cnt <= kActNbrCap` against `<` in the greedy step (a
full list and the rescan of the cells visit the same earlier candidates), and `hessian == 0` setting `stop` (a zero Hessian makes the step
0 / 0 or b / 0, no target is valid at such an inverse depth, and `n_valid == 0` sets `stop` itself)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import activation_model as am
import activation_scenes as asc

pytestmark = pytest.mark.gpu


def _check_selection(sc, m, out):
    """statuses, counts, distance and the set states as the model has them"""
    st, idp, res, states = out
    assert res["number_of_active_points"] == m.n_active
    if sc["exact"]:
        assert res["min_distance_to_neighbor"] == m.distance, (res["min_distance_to_neighbor"], m.distance)
    else:
        assert abs(res["min_distance_to_neighbor"] - m.distance) < 1e-12
    assert len(st) == len(m.statuses)
    for k, (a, b) in enumerate(zip(m.statuses, st)):
        assert np.array_equal(a, b), (sc["name"], k, np.flatnonzero(a != b), a[a != b], b[a != b])
    tot = np.concatenate(m.statuses) if m.statuses else np.zeros(0)
    assert (res["n_activated"], res["n_skipped"], res["n_deleted"]) == ((tot == am.ACTIVATE).sum(), (tot == am.SKIP).sum(), (tot == am.DELETE).sum())
    n_immature = len(tot)
    assert 1 <= res["selection_rounds"] <= n_immature + 1
    if sc["name"].startswith("chain"):   # (no exact count: it depends on which stores of a round the others happen to see)
        assert 2 <= res["selection_rounds"]
    for state_m, state_g in zip(m.states, states):
        assert (state_m is None) == (state_g is None)
        if state_m is not None:
            assert np.array_equal(state_m["status"], state_g["status"])


def _check_refined(m, out, rtol=1e-9):
    _, idp, _, states = out
    for state_m, state_g, mid_m, mid_g in zip(m.states, states, m.idepth, idp):
        assert len(mid_m) == len(mid_g)
        if state_m is None or len(mid_m) == 0:
            continue
        for key in ("idepth_min", "idepth_max"):
            assert np.abs(state_m[key] - state_g[key]).max() <= rtol * max(1.0, np.abs(state_m[key]).max()), key
        assert np.abs(mid_m - mid_g).max() <= rtol * max(1.0, np.abs(mid_m).max())


@pytest.mark.parametrize("name", asc.SELECTION_NAMES)
def test_selection_f64(name):
    sc = asc.scenes("selection")[name]
    m = asc.model(sc)
    out = asc.run_scene_gpu(sc)
    _check_selection(sc, m, out)
    _check_refined(m, out, 0.0)   # no refinement: intervals untouched, idepth() returned as it is


@pytest.mark.parametrize("name", asc.SELECTION_NAMES)
def test_selection_f32_pyramids(name):
    """the selection reads no intensity: identical with float texels"""
    from dsopp_amd import capi
    sc = asc.scenes("selection")[name]
    _check_selection(sc, asc.model(sc), asc.run_scene_gpu(sc, dtype=capi.F32))


@pytest.mark.parametrize("name", asc.REFINEMENT_NAMES)
def test_refinement_f64(name):
    sc = asc.scenes("refinement")[name]
    m = asc.model(sc)
    out = asc.run_scene_gpu(sc)
    _check_selection(sc, m, out)
    _check_refined(m, out)


@pytest.mark.parametrize("name", asc.REFINEMENT_NAMES)
def test_refinement_f32_pyramids(name):
    """float texels: at least 99 % of the statuses as the model has them, inverse depths to 2e-4 relative on the landmarks both keep"""
    from dsopp_amd import capi
    sc = asc.scenes("refinement")[name]
    m = asc.model(sc)
    st, idp, res, _ = asc.run_scene_gpu(sc, dtype=capi.F32)
    assert res["number_of_active_points"] == m.n_active
    same = np.concatenate(m.statuses) == np.concatenate(st)
    print(name, "statuses equal: %.4f" % same.mean())
    assert same.mean() >= 0.99
    for a, b, mid_m, mid_g in zip(m.statuses, st, m.idepth, idp):
        keep = (a == am.ACTIVATE) & (b == am.ACTIVATE)
        if keep.any():
            assert np.abs(mid_m[keep] - mid_g[keep]).max() <= 2e-4 * np.abs(mid_m[keep]).max()


def test_scan_all_fallback_on_chains_clusters_and_the_work_list_boundary():
    """DSOPP_HIP_ACT_WORK_CAP=8 (read once per process): the greedy rounds may list 8 undecided candidates.  workcap_8 leaves exactly 8 (the
    list, full), workcap_9 exactly 9 and the chains and clusters far more: rounds that scan every candidate"""
    env = dict(os.environ, DSOPP_HIP_ACT_WORK_CAP="8")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-k", "test_selection_f64 and (chain or cluster or workcap)"],
                       env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "8 passed" in r.stdout and "failed" not in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_scratch_reuse_across_calls_of_different_size():
    """the window keeps the activator's work buffers between calls: a large call, one with nothing at all, a small one and the large one again on
    ONE window, each equal to the same call on a fresh window (and to the model)"""
    from dsopp_amd import capi
    large = asc.scenes("selection")["counts_large"]          # keyframes with (257 active, 257 immature), (0, no set), (257, 1)
    frames, intr = large["frames"], large["intr"]
    rng = np.random.default_rng(3)
    small_set = asc.immature_at(np.stack([rng.integers(16, 237, 5) / 4.0, rng.integers(16, 173, 5) / 4.0], axis=1))
    middle = lambda immature: [dict(frames[1], immature=immature), frames[-1]]   # noqa: E731  (the keyframe without active landmarks, alone)
    calls = [("large", frames, [0, 1, 2]), ("empty", middle(None), [1]), ("small", middle(small_set), [1]), ("large again", frames, [0, 1, 2])]
    g = capi.HipWindow(capi.default_pba_options())
    for s in asc.load_gpu(g, frames, intr):
        if s is not None:
            s.close()
    pyr = asc.newest_pyramid(frames, None, capi.F64)
    for label, fr, ids in calls:
        sc = dict(large, name="reuse " + label, frames=fr, desired=sum(len(f["active_idepth"]) for f in fr[:-1]))
        sets = []
        for f in fr[:-1]:
            sets.append(None if f["immature"] is None else capi.ImmatureSet(f["immature"]))
            if sets[-1] is not None:
                sets[-1].upload(f["immature"])
        reused = asc.activate_gpu(g, fr, sets, pyr, sc["desired"], sc["dist0"], False, ids=ids)
        for s in sets:
            if s is not None:
                s.close()
        fresh = asc.run_scene_gpu(sc)
        m = asc.model(sc)
        _check_selection(sc, m, fresh)
        _check_selection(sc, m, reused)
        for a, b in zip(fresh[1], reused[1]):
            assert np.array_equal(a, b), label
        assert dict(fresh[2], selection_rounds=0) == dict(reused[2], selection_rounds=0), (label, fresh[2], reused[2])
    pyr.close()
    g.close()
