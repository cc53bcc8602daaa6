"""GPU parity tests of the sliding-window photometric BA: the HIP path (through the C-ABI) against the CPU oracle on
identical seeded synthetic windows, stage by stage (SURVEY.md §8d parity bar):
   residual energies / statuses   rel <= 1e-9 (f64 path)
   H / b entries                  |d| <= 1e-9 |x| + 1e-9 ||H||_max  (bar: 1e-6)
   pose update                    ||d_xi_gpu - d_xi_cpu||_inf <= 1e-9  (bar: 1e-5, BASELINE.json)
   idepth steps                   rel 1e-7 (bar: 1e-4)
"""
import numpy as np
import pytest

from dsopp_amd import synthetic as syn

pytestmark = pytest.mark.gpu


def _both(win, **opts):
    from dsopp_amd import capi
    from oracle import pyoracle as po
    o = po.OracleWindow(po.default_pba_options(**opts))
    syn.load_window(o, win)
    g = capi.HipWindow(capi.default_pba_options(**opts))
    syn.load_window(g, win)
    return o, g


def _close(a, b, rtol, atol):
    return np.abs(np.asarray(a) - np.asarray(b)).max() <= atol + rtol * np.abs(np.asarray(b)).max()


@pytest.mark.parametrize("fej", [1, 0])
def test_stage_parity_small(small_window, fej):
    win = small_window
    o, g = _both(win, first_estimate_jacobians=fej)
    o.begin()
    g.begin()
    eo, no = o.calculate_energy()
    eg, ng = g.calculate_energy()
    assert no == ng
    assert abs(eo - eg) <= 1e-10 * abs(eo)
    for fr in win.frames:
        for ft in win.frames:
            if fr.frame_id == ft.frame_id:
                continue
            ro = o.get_residuals(fr.frame_id, ft.frame_id)
            rg = g.get_residuals(fr.frame_id, ft.frame_id)
            assert np.array_equal(ro["candidate"], rg["candidate"])
            assert _close(rg["energy"], ro["energy"], 1e-10, 1e-9)
    o.linearize()
    g.linearize()
    so, sg = o.get_system(), g.get_system()
    names = ["H_pp", "b_pp", "H_schur", "b_schur"]
    for name, a, b in zip(names, sg, so):
        scale = np.abs(b).max()
        if name == "H_pp":  # 1e16 fixed-frame prior dominates the max: compare the free part against its own scale too
            assert np.abs(a[8:, 8:] - b[8:, 8:]).max() <= 1e-9 * np.abs(b[8:, 8:]).max(), name
        assert np.abs(a - b).max() <= 1e-9 * scale, name
    lam = 1e-5
    st_o = o.calculate_step(lam)
    st_g = g.calculate_step(lam)
    assert np.abs(st_o - st_g).max() <= 1e-9, np.abs(st_o - st_g).max()
    for f in win.frames:
        lo, lg = o.get_landmarks(f.frame_id), g.get_landmarks(f.frame_id)
        assert _close(lg["idepth_step"], lo["idepth_step"], 1e-7, 1e-12)
        assert _close(lg["hpib"], lo["hpib"], 1e-9, 1e-9)
        assert _close(lg["b_d"], lo["b_d"], 1e-9, 1e-9)
        assert _close(lg["inv_hdd"], lo["inv_hdd"], 1e-9, 0)
    e1o, n1o = o.calculate_energy()
    e1g, n1g = g.calculate_energy()
    assert n1o == n1g and abs(e1o - e1g) <= 1e-9 * abs(e1o)
    ao, ag = o.accept_step(), g.accept_step()
    assert abs(ao[0] - ag[0]) <= 1e-10 * ao[0] and abs(ao[1] - ag[1]) <= 1e-7 * ao[1]
    for f in win.frames:
        so_, sg_ = o.get_frame_state(f.frame_id), g.get_frame_state(f.frame_id)
        for a, b in zip(sg_, so_):
            assert np.abs(a - b).max() <= 1e-9
        assert _close(g.get_landmarks(f.frame_id, False)["idepth"], o.get_landmarks(f.frame_id)["idepth"], 1e-9, 1e-12)
    # second iteration from the accepted state (exercises status promotion + pair-constant reuse)
    o.linearize()
    g.linearize()
    st_o, st_g = o.calculate_step(lam), g.calculate_step(lam)
    assert np.abs(st_o - st_g).max() <= 1e-8
    e2o, _ = o.calculate_energy()
    e2g, _ = g.calculate_energy()
    assert abs(e2o - e2g) <= 1e-8 * abs(e2o)
    o.reject_step()
    g.reject_step()
    e3o, _ = o.calculate_energy()
    e3g, _ = g.calculate_energy()
    assert abs(e3o - e3g) <= 1e-9 * abs(e3o) and abs(e3g - e1g) <= 1e-9 * abs(e1g)
    g.close()


@pytest.mark.parametrize("host_driven", [0, 1])
def test_full_solve_parity(small_window, host_driven):
    """solve() with the LM control flow on the device (default) and on the host: both must reproduce the oracle."""
    win = small_window
    o, g = _both(win)
    g.set_lm_mode(host_driven)
    eo, ito, nvo = o.solve()
    eg, itg, nvg = g.solve()
    assert ito == itg and nvo == nvg
    assert abs(eo - eg) <= 1e-7 * abs(eo)
    for f in win.frames:
        To, abo = o.get_pose(f.frame_id)
        Tg, abg = g.get_pose(f.frame_id)
        assert np.abs(To - Tg).max() <= 1e-7, (f.frame_id, np.abs(To - Tg).max())  # bar: 1e-5
        assert np.abs(abo - abg).max() <= 1e-7
        lo, lg = o.get_landmarks(f.frame_id), g.get_landmarks(f.frame_id, False)
        assert _close(lg["idepth"], lo["idepth"], 1e-6, 1e-9)
        assert np.array_equal(lo["flags"] & 3, lg["flags"] & 3)
        assert np.array_equal(lo["n_inliers"], lg["n_inliers"])
        assert _close(lg["relative_baseline"], lo["relative_baseline"], 1e-6, 1e-9)
    for fr in win.frames:
        for ft in win.frames:
            if fr.frame_id != ft.frame_id:
                assert np.array_equal(o.get_residuals(fr.frame_id, ft.frame_id)["status"], g.get_residuals(fr.frame_id, ft.frame_id)["status"])
                co, cg = o.get_covariance(fr.frame_id, ft.frame_id), g.get_covariance(fr.frame_id, ft.frame_id)
                assert np.abs(co - cg).max() <= 1e-4 * np.abs(co).max()  # reference's own Eigen-vs-Ceres bar: rel 1e-2
    g.close()


def test_float_storage_mode(small_window):
    """F32 evaluation (the reference's -DUSE_FLOAT build) with fp64 accumulation: looser bar, fp32 round-off class."""
    from dsopp_amd import capi
    from oracle import pyoracle as po
    win = small_window
    o = po.OracleWindow(po.default_pba_options())
    syn.load_window(o, win)
    g = capi.HipWindow(capi.default_pba_options(dtype=capi.F32))
    syn.load_window(g, win)
    o.begin()
    g.begin()
    eo, no = o.calculate_energy()
    eg, ng = g.calculate_energy()
    assert abs(no - ng) <= 2 and abs(eo - eg) <= 1e-4 * abs(eo)
    o.linearize()
    g.linearize()
    st_o, st_g = o.calculate_step(1e-5), g.calculate_step(1e-5)
    assert np.abs(st_o - st_g).max() <= 1e-3 * max(1e-2, np.abs(st_o).max())
    g.close()
