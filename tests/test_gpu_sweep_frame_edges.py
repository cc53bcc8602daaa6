"""The window's sweeps against the CPU oracle where the rest of the suite never takes them (scenes: tests/sweep_edge_scenes.py, checked
on the oracle alone by tests/test_sweep_edge_scenes.py):
  frame sizes that are no multiple of four     row stride (W + 3) / 4 and allocation of the tiled intensity plane, f64 (4 x 2) and f32 (4 x 4)
  keyframes of different sizes in one window   reference and target width / height / plane stride are separate kernel arguments
  frames borrowed at pyramid level 1 and 2     FrameDev::level: view(level), intensityPlane(level), itilesX(level)
  landmarks down to 2 pixels from the border   the inclusive ROI limits 4 and W - 5 on the reference side, the target side and in the
                                               first-estimate-Jacobians item test
  intensities through a photometric LUT        the plane's cleared lowest mantissa bit is set in the texels
calculate_energy (and the energy halves of optimize) read the intensity plane, linearize reads the texels: both are held to the same oracle.
No tolerance is new here; every bar names the test it was taken from.
"""
import functools

import numpy as np
import pytest

import sweep_edge_scenes as ses

pytestmark = pytest.mark.gpu

_PERMUTED = ("mixed-permuted", functools.partial(ses.mixed, ses.MIXED_SIZES_PERMUTED))
_F64 = pytest.mark.parametrize("name,builder", ses.F64_SCENES + [_PERMUTED], ids=[s[0] for s in ses.F64_SCENES + [_PERMUTED]])
_F32 = pytest.mark.parametrize("name,builder", ses.F32_SCENES, ids=[s[0] for s in ses.F32_SCENES])


def _both(scene, dtype=None, **opts):
    """the oracle and the HIP window loaded with one scene; the device pyramids the HIP window borrows (level scenes) to close afterwards"""
    from dsopp_amd import capi
    from oracle import pyoracle as po
    o = ses.load(po.OracleWindow(po.default_pba_options(**opts)), scene)
    if dtype is not None:
        opts = dict(opts, dtype=dtype)
    pyramids = ses.build_pyramids(scene, capi.F64 if dtype is None else dtype)
    g = ses.load(capi.HipWindow(capi.default_pba_options(**opts)), scene, pyramids)
    return o, g, pyramids


def _close_all(o, g, pyramids):
    g.close()
    o.close()
    for p in pyramids or ():
        p.close()


def _close(a, b, rtol, atol):
    return np.abs(np.asarray(a) - np.asarray(b)).max() <= atol + rtol * np.abs(np.asarray(b)).max()


@_F64
@pytest.mark.parametrize("fej", [1, 0])
def test_stage_parity(name, builder, fej):
    """the sequence and the bars of test_gpu_pba.py::test_stage_parity_small, with the residual statuses compared as well"""
    scene = builder()
    frames = scene.window.frames
    o, g, pyramids = _both(scene, first_estimate_jacobians=fej)
    o.begin()
    g.begin()
    eo, no = o.calculate_energy()
    eg, ng = g.calculate_energy()
    assert no == ng
    assert abs(eo - eg) <= 1e-10 * abs(eo)
    for r, t in ses.pairs(scene):
        ro, rg = o.get_residuals(r, t), g.get_residuals(r, t)
        assert np.array_equal(ro["status"], rg["status"]), (r, t)
        assert np.array_equal(ro["candidate"], rg["candidate"]), (r, t, np.flatnonzero(ro["candidate"] != rg["candidate"]))
        assert _close(rg["energy"], ro["energy"], 1e-10, 1e-9)
    o.linearize()
    g.linearize()
    so, sg = o.get_system(), g.get_system()
    for sysname, a, b in zip(["H_pp", "b_pp", "H_schur", "b_schur"], sg, so):
        scale = np.abs(b).max()
        if sysname == "H_pp":  # 1e16 fixed-frame prior dominates the max: compare the free part against its own scale too
            assert np.abs(a[8:, 8:] - b[8:, 8:]).max() <= 1e-9 * np.abs(b[8:, 8:]).max(), sysname
        assert np.abs(a - b).max() <= 1e-9 * scale, sysname
    lam = 1e-5
    st_o, st_g = o.calculate_step(lam), g.calculate_step(lam)
    assert np.abs(st_o - st_g).max() <= 1e-9, np.abs(st_o - st_g).max()
    for f in frames:
        lo, lg = o.get_landmarks(f.frame_id), g.get_landmarks(f.frame_id)
        assert _close(lg["idepth_step"], lo["idepth_step"], 1e-7, 1e-12)
        assert _close(lg["hpib"], lo["hpib"], 1e-9, 1e-9)
        assert _close(lg["b_d"], lo["b_d"], 1e-9, 1e-9)
        assert _close(lg["inv_hdd"], lo["inv_hdd"], 1e-9, 0)
    e1o, n1o = o.calculate_energy()
    e1g, n1g = g.calculate_energy()
    assert n1o == n1g and abs(e1o - e1g) <= 1e-9 * abs(e1o)
    for r, t in ses.pairs(scene):   # the candidates of the stepped state: landmarks near a limit cross it here
        assert np.array_equal(o.get_residuals(r, t)["candidate"], g.get_residuals(r, t)["candidate"]), (r, t)
    ao, ag = o.accept_step(), g.accept_step()
    assert abs(ao[0] - ag[0]) <= 1e-10 * ao[0] and abs(ao[1] - ag[1]) <= 1e-7 * ao[1]
    for f in frames:
        for a, b in zip(g.get_frame_state(f.frame_id), o.get_frame_state(f.frame_id)):
            assert np.abs(a - b).max() <= 1e-9
        assert _close(g.get_landmarks(f.frame_id, False)["idepth"], o.get_landmarks(f.frame_id)["idepth"], 1e-9, 1e-12)
    # second iteration from the accepted state (status promotion + pair-constant reuse)
    o.linearize()
    g.linearize()
    st_o, st_g = o.calculate_step(lam), g.calculate_step(lam)
    assert np.abs(st_o - st_g).max() <= 1e-8
    e2o, _ = o.calculate_energy()
    e2g, _ = g.calculate_energy()
    assert abs(e2o - e2g) <= 1e-8 * abs(e2o)
    for r, t in ses.pairs(scene):
        assert np.array_equal(o.get_residuals(r, t)["status"], g.get_residuals(r, t)["status"]), (r, t)
    _close_all(o, g, pyramids)


def _compare_optimize(o, g, scene):
    """optimize() of both under the bars of test_gpu_pba_edge.py::_compare_solve"""
    eo, ito, nvo = o.optimize()
    eg, itg, nvg = g.optimize()
    assert (ito, nvo) == (itg, nvg)
    assert ito >= 2
    assert abs(eo - eg) <= 1e-7 * max(abs(eo), 1e-30)
    for f in scene.window.frames:
        To, abo = o.get_pose(f.frame_id)
        Tg, abg = g.get_pose(f.frame_id)
        assert np.abs(To - Tg).max() <= 1e-7, (f.frame_id, np.abs(To - Tg).max())
        assert np.abs(abo - abg).max() <= 1e-7
        lo, lg = o.get_landmarks(f.frame_id), g.get_landmarks(f.frame_id, False)
        assert np.abs(lg["idepth"] - lo["idepth"]).max() <= 1e-6 * np.abs(lo["idepth"]).max() + 1e-9
        assert np.array_equal(lo["flags"] & 3, lg["flags"] & 3)
        assert np.array_equal(lo["n_inliers"], lg["n_inliers"])
    for r, t in ses.pairs(scene):
        assert np.array_equal(o.get_residuals(r, t)["status"], g.get_residuals(r, t)["status"]), (r, t)


@_F64
@pytest.mark.parametrize("lm_mode", [0, 1])
def test_full_solve(name, builder, lm_mode):
    """the LM loop on the device (fused, lm_mode 0) and driven from the host (lm_mode 1)"""
    scene = builder()
    o, g, pyramids = _both(scene)
    g.set_lm_mode(lm_mode)
    _compare_optimize(o, g, scene)
    _close_all(o, g, pyramids)


def test_permuted_sizes_change_what_the_oracle_decides():
    """the swap detector of the mixed scene: test_stage_parity / test_full_solve hold the HIP window to the oracle on the same keyframes
    under two assignments of the sizes; that pins every size to its frame only if the oracle itself tells the two assignments apart"""
    from oracle import pyoracle as po
    cands = []
    for sizes in (ses.MIXED_SIZES, ses.MIXED_SIZES_PERMUTED):
        scene = ses.mixed(sizes)
        o = ses.load(po.OracleWindow(po.default_pba_options()), scene)
        o.optimize()
        cands.append(np.concatenate([o.get_residuals(r, t)["candidate"] for r, t in ses.pairs(scene)]))
        o.close()
    assert (cands[0] != cands[1]).sum() >= 1


@_F32
def test_f32_energy_and_full_solve(name, builder):
    """fp32 storage and evaluation (4 x 4 tiles of the intensity plane: rows of tiles (H + 3) / 4) against the fp64 oracle: energy and
    valid count after begin() with the bars of test_gpu_masks.py::test_pba_masked_window_full_size_f32, then the full solve with those of
    test_gpu_pba_edge.py::test_float_mode_full_solve"""
    from dsopp_amd import capi
    scene = builder()
    o, g, pyramids = _both(scene, dtype=capi.F32)
    o.begin()
    g.begin()
    eo, no = o.calculate_energy()
    eg, ng = g.calculate_energy()
    assert abs(no - ng) <= 2 and abs(eo - eg) <= 1e-4 * abs(eo), (no, ng, eo, eg)
    eo, ito, nvo = o.optimize()
    eg, itg, nvg = g.optimize()
    assert ito == itg and abs(nvo - nvg) <= 3, (ito, itg, nvo, nvg)
    assert abs(eo - eg) <= 2e-3 * abs(eo)
    for f in scene.window.frames:
        To, _ = o.get_pose(f.frame_id)
        Tg, _ = g.get_pose(f.frame_id)
        assert np.abs(To - Tg).max() <= 2e-4, np.abs(To - Tg).max()
    _close_all(o, g, pyramids)
