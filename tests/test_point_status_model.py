"""tests/point_status_model.py against the CPU oracle's updatePointStatuses on a window whose energies have an upper tail, with everything
the rule branches on present at once: landmarks flagged marginalised or outlier at upload, connections preset to OUTLIER / OCCLUDED / OOB,
and one keyframe marked marginalised before the call.  Statuses, energies, inlier counts and flags are equalities; the relative baseline
is held to the model's bound.  This is what entitles the model to judge the device (tests/test_gpu_point_statuses.py)."""
import numpy as np
import pytest

import point_status_model as psm
from dsopp_amd import synthetic as syn


def _oracle_before_and_after(win, sigma, statuses, flags, marginalize):
    from oracle import pyoracle as po
    o = psm.load(po.OracleWindow(po.default_pba_options(sigma_huber_loss=sigma)), win, statuses, flags)
    o.begin()
    o.calculate_energy()
    o.linearize()
    ids = [f.frame_id for f in win.frames]
    marginalized = {r: False for r in ids}
    if marginalize is not None:
        o.mark_frame_marginalized(marginalize)
        marginalized[marginalize] = True
    before = psm.read_tables(o, ids)
    o.update_point_statuses()
    after = psm.read_tables(o, ids)
    return ids, marginalized, before, after


@pytest.mark.parametrize("sigma,seed", [(20.0, 4), (3.0, 5)])
def test_model_equals_the_oracle_on_a_window_with_a_tail(sigma, seed):
    win = syn.make_window(num_frames=4, num_points=360, width=320, height=240, seed=seed)
    statuses, flags = psm.presets(win, psm.corrupt(win, seed))
    victim = win.frames[2].frame_id                  # not the fixed frame
    assert not win.frames[2].fixed
    ids, marginalized, (res, lms, centres), (res_after, lms_after, _) = _oracle_before_and_after(win, sigma, statuses, flags, victim)
    want = psm.update_point_statuses(ids, res, lms, marginalized, centres, sigma)
    # the input exercises every branch of the rule
    n_ok = sum(int((v["status"] == psm.OK).sum()) for v in res.values())
    assert 0 < want.n_select < n_ok                               # marginalised landmarks and the marginalised target hold OK residuals that stay out
    assert 0 < want.n_outliers < want.n_select // 4 + 1
    assert any(np.any((lms[r]["flags"] & psm.FLAG_MARGINALIZED) != 0) for r in ids)
    assert any(np.any((want.landmarks[r]["flags"] & ~lms[r]["flags"] & psm.FLAG_OUTLIER) != 0) for r in ids)   # a landmark lost its last inlier
    assert any(np.any(v["status"] > psm.OUTLIER) for v in res.values())
    bad, worst = psm.mismatches(want, res_after, lms_after)
    assert not bad, "\n".join(bad)
    print(f"sigma {sigma}: {n_ok} OK, {want.n_select} selected from, rank {want.rank}, {want.n_outliers} outliers; "
          f"relative baseline at most {worst * psm.BASELINE_FACTOR:.4f} eps idepth (|c_r| + |c_t|) from the model")
    # what the call must leave alone, bit for bit: marginalised landmarks, and the tables towards the marginalised target
    for r in ids:
        gone = (lms[r]["flags"] & psm.FLAG_MARGINALIZED) != 0
        for k in ("relative_baseline", "n_inliers", "flags"):
            assert np.array_equal(lms_after[r][k][gone], lms[r][k][gone]), (r, k)
        for t in ids:
            if t != r:
                keep = np.ones(len(gone), dtype=bool) if t == victim else gone
                for k in ("status", "energy"):
                    assert np.array_equal(res_after[(r, t)][k][keep], res[(r, t)][k][keep]), (r, t, k)


def test_model_without_an_eligible_residual():
    """every connection preset to a non-OK status: the threshold is 0 and only residuals with a positive stale energy change"""
    win = syn.make_window(num_frames=3, num_points=90, width=320, height=240, seed=4)
    psm.corrupt(win, 4)
    statuses = {(a.frame_id, b.frame_id): np.full(len(a.uv), psm.OUTLIER + (i + j) % 3, dtype=np.uint8)
                for i, a in enumerate(win.frames) for j, b in enumerate(win.frames) if i != j}
    ids, marginalized, (res, lms, centres), (res_after, lms_after, _) = _oracle_before_and_after(win, 20.0, statuses, None, None)
    want = psm.update_point_statuses(ids, res, lms, marginalized, centres, 20.0)
    assert want.n_select == 0 and want.threshold == 0.0 and want.selected is None and want.n_outliers == 0
    bad, _ = psm.mismatches(want, res_after, lms_after)
    assert not bad, "\n".join(bad)
    for r in ids:
        assert np.all(lms_after[r]["n_inliers"] == 0) and np.all((lms_after[r]["flags"] & psm.FLAG_OUTLIER) != 0)


def test_model_pieces():
    ids = [7, 9]
    res = {(7, 9): dict(status=np.array([0, 0, 0, 2, 0], np.uint8), energy=np.array([1.0, 5.0, 3.0, 9.0, 2.0])),
           (9, 7): dict(status=np.zeros(0, np.uint8), energy=np.zeros(0))}
    lms = {7: dict(idepth=np.full(5, 0.5), relative_baseline=np.array([0.0, 0.0, 4.0, 0.0, 0.0]), flags=np.array([0, 0, 0, 0, 1], np.uint8),
                   n_inliers=np.full(5, 3)),
           9: dict(idepth=np.zeros(0), relative_baseline=np.zeros(0), flags=np.zeros(0, np.uint8), n_inliers=np.zeros(0, np.int32))}
    centres = {7: np.array([0.0, 0.0, 0.0]), 9: np.array([3.0, 4.0, 0.0])}
    w = psm.update_point_statuses(ids, res, lms, {7: False, 9: False}, centres, 2.0)
    # three energies enter (the OCCLUDED one and the marginalised landmark's stay out): rank int(2.25) = 2 -> 5.0, + 2
    assert (w.n_select, w.rank, w.selected, w.threshold) == (3, 2, 5.0, 7.0)
    assert w.residuals[(7, 9)]["status"].tolist() == [0, 0, 0, 1, 0] and w.residuals[(7, 9)]["energy"].tolist() == [1.0, 5.0, 3.0, 0.0, 2.0]
    assert w.n_outliers == 0                                      # the OCCLUDED residual became OUTLIER, no OK one did
    assert w.landmarks[7]["n_inliers"].tolist() == [1, 1, 1, 0, 3]   # the marginalised landmark keeps its count
    assert w.landmarks[7]["relative_baseline"].tolist() == [2.5, 2.5, 4.0, 0.0, 0.0]
    assert w.landmarks[7]["flags"].tolist() == [0, 0, 0, 2, 1]
    # a marginalised target: nothing enters, nothing changes but the outlier bits of landmarks left without a residual
    w = psm.update_point_statuses(ids, res, lms, {7: False, 9: True}, centres, 2.0)
    assert w.n_select == 0 and w.threshold == 0.0
    assert w.residuals[(7, 9)]["status"].tolist() == [0, 0, 0, 2, 0] and w.landmarks[7]["flags"].tolist() == [2, 2, 2, 2, 1]
    assert psm.sharpness([1.0, 5.0, 3.0], 2, 2.0) == (0.0, np.inf) and psm.sharpness([1.0, 5.0, 3.0, 8.0], 2, 2.0) == (0.0, 1.0)
