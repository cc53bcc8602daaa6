"""tests/sweep_f32_model.py held to account on the CPU: its central values against the fp64 oracle, the share of items its margins leave
undecided, and its comparison against six deliberate mistakes (no GPU needed).

  model against the oracle   with u = 2^-53 and float64 texels the model's central values are the oracle's on every scene of F64_SCENES,
                             first-estimate Jacobians on and off, under the bars of test_gpu_pba.py::test_stage_parity_small (statuses and
                             candidates equal, energies 1e-10 / 1e-9, system blocks 1e-9, landmark quantities 1e-9), at the initial state
                             and at the state of the oracle's first step: a wrong formula cannot hide behind its own bound
  undecided share            at most 1 % of the items of each fp32 scene, in the residual-only and in the linearisation sweep
  defects                    compare() fails on the model's own central values computed with each of DEFECTS, and passes on the clean ones

Measured here: 0 undecided items of 480 in every scene, sweep and mode; every defect is rejected on at least the masked scene (the mask
lookup and b_t show nowhere else: no other scene has a mask or a non-zero affine state), the other four on all 24 (scene, mode) cases.
"""
import functools

import numpy as np
import pytest

import sweep_edge_scenes as ses
import sweep_f32_model as sm

_F64 = pytest.mark.parametrize("name,builder", ses.F64_SCENES, ids=[s[0] for s in ses.F64_SCENES])
_F32 = pytest.mark.parametrize("name,builder", ses.F32_EDGE_SCENES, ids=[s[0] for s in ses.F32_EDGE_SCENES])
UNDECIDED_CAP = 0.01
LAMBDA = 1e-5


def _close(a, b, rtol, atol):
    return np.abs(np.asarray(a) - np.asarray(b)).max() <= atol + rtol * np.abs(np.asarray(b)).max()


@functools.lru_cache(maxsize=None)
def _oracle_step(builder, fej):
    """(eps + step per frame, inverse-depth steps per frame) of the oracle's first step: a state off the linearisation point"""
    from oracle import pyoracle as po
    scene = builder()
    o = ses.load(po.OracleWindow(po.default_pba_options(first_estimate_jacobians=fej)), scene)
    o.begin()
    o.calculate_energy()
    o.linearize()
    o.calculate_step(LAMBDA)
    frames = scene.window.frames
    step = np.stack([o.get_frame_state(f.frame_id)[3] for f in frames])
    dsteps = [o.get_landmarks(f.frame_id)["idepth_step"].copy() for f in frames]
    o.close()
    return step, dsteps


def _stepped(scene, builder, fej):
    step, dsteps = _oracle_step(builder, fej)
    st = sm.initial_state(scene)
    st.step[:] = step
    st.idepth_step = [d.copy() for d in dsteps]
    return st


@_F64
@pytest.mark.parametrize("fej", [1, 0])
def test_model_equals_oracle(name, builder, fej):
    from oracle import pyoracle as po
    scene = builder()
    frames = scene.window.frames
    win = sm.model_window(scene, f32=False)
    st0 = sm.initial_state(scene)
    o = ses.load(po.OracleWindow(po.default_pba_options(first_estimate_jacobians=fej)), scene)
    o.begin()
    eo, no = o.calculate_energy()
    statuses = sm.push_statuses(win, st0, fej, u=sm.U64)
    me = sm.sweep(win, st0, fej, u=sm.U64, statuses=statuses)
    assert me.undecided == 0 and me.count == (no, no)
    assert abs(eo - me.energy.v) <= 1e-10 * abs(eo)
    for r, t in ses.pairs(scene):
        ro, p = o.get_residuals(r, t), me.pairs[(r, t)]
        assert np.array_equal(ro["status"], p["status"]), (r, t)
        assert np.array_equal(ro["candidate"], p["candidate"]), (r, t, np.flatnonzero(ro["candidate"] != p["candidate"]))
        assert _close(np.where(p["evaluate"], p["energy"].v, 0.0), ro["energy"], 1e-10, 1e-9)
        assert _close(np.where(p["evaluate"], p["weight"], 1.0), np.where(p["evaluate"], ro["huber_weight"], 1.0), 1e-10, 0)
    o.linearize()
    ml = sm.sweep(win, st0, fej, linearize=True, u=sm.U64, statuses=statuses)
    assert ml.undecided == 0 and sm.unbounded(ml) == 0
    for sysname, a, b in zip(["H_pp", "b_pp", "H_schur", "b_schur"], [x.v for x in ml.system], o.get_system()):
        if sysname == "H_pp":
            assert np.abs(a[8:, 8:] - b[8:, 8:]).max() <= 1e-9 * np.abs(b[8:, 8:]).max(), sysname
        assert np.abs(a - b).max() <= 1e-9 * np.abs(b).max(), sysname
    o.calculate_step(LAMBDA)
    for i, f in enumerate(frames):
        lo, lm = o.get_landmarks(f.frame_id), ml.landmarks[i]
        assert _close(lm["hpib"].v, lo["hpib"], 1e-9, 1e-9)
        assert _close(lm["b_d"].v, lo["b_d"], 1e-9, 1e-9)
        assert _close(lm["inv_hdd"].v, lo["inv_hdd"], 1e-9, 0)
    # the stepped state: pair constants from eps + step, inverse depths from idepth + idepth_step, the snapshot stays
    e1o, n1o = o.calculate_energy()
    m1 = sm.sweep(win, _stepped(scene, builder, fej), fej, u=sm.U64, fej_idepth=st0.idepth, statuses=statuses)
    assert m1.count == (n1o, n1o) and abs(e1o - m1.energy.v) <= 1e-9 * abs(e1o)
    for r, t in ses.pairs(scene):
        ro, p = o.get_residuals(r, t), m1.pairs[(r, t)]
        assert np.array_equal(ro["candidate"], p["candidate"]), (r, t)
        assert _close(np.where(p["evaluate"], p["energy"].v, 0.0), ro["energy"], 1e-9, 1e-9)
    o.close()


@functools.lru_cache(maxsize=None)
def _f32_results(builder, fej, defect=None, stepped=False):
    """(residual-only sweep, linearisation sweep) of the f32 model; stepped: the residual-only sweep at the oracle's first step"""
    scene = builder()
    win = sm.model_window(scene)
    st0 = sm.initial_state(scene)
    statuses = sm.push_statuses(win, st0, fej, defect=defect)
    if stepped:
        return sm.sweep(win, _stepped(scene, builder, fej), fej, defect=defect, fej_idepth=st0.idepth, statuses=statuses), None
    return (sm.sweep(win, st0, fej, defect=defect, statuses=statuses),
            sm.sweep(win, st0, fej, linearize=True, defect=defect, statuses=statuses))


@_F32
@pytest.mark.parametrize("fej", [1, 0])
def test_undecided_share(name, builder, fej):
    me, ml = _f32_results(builder, fej)
    m1, _ = _f32_results(builder, fej, stepped=True)
    for what, m in (("energy", me), ("linearize", ml), ("stepped energy", m1)):
        print(f"{name} fej={fej} {what}: {m.undecided} of {m.items} items undecided")
        assert m.items == 2 * ses.NUM_FRAMES * ses.PER_FRAME
        assert m.undecided <= UNDECIDED_CAP * m.items, (what, m.undecided)
    if me.undecided == 0 and ml.undecided == 0:
        assert sm.unbounded(ml) == 0
        for x in ml.system:
            assert np.isfinite(x.e).all()


@_F32
def test_clean_values_pass(name, builder):
    for fej in (1, 0):
        me, ml = _f32_results(builder, fej)
        fails, ratios = sm.compare(sm.as_device(me, ml), me, ml)
        assert not fails, fails
        assert max(ratios.values()) == 0.0
        m1, _ = _f32_results(builder, fej, stepped=True)
        fails, _ = sm.compare(sm.as_device(m1), m1)
        assert not fails, fails


def test_masked_scene_masks_part_of_a_pattern():
    """the masked scene is what it is for: items lost to the mask alone, some of them with only part of their pattern masked"""
    scene = ses.masked_border()
    unmasked = ses.border(*ses.SIZES[0])
    win = sm.model_window(scene)
    me = sm.sweep(win, sm.initial_state(scene), 1)
    plain = sm.model_window(scene)
    for f in plain.frames:
        f.mask = None
    mp = sm.sweep(plain, sm.initial_state(scene), 1)
    lost = sum(int((mp.pairs[k]["ok"] & ~me.pairs[k]["ok"]).sum()) for k in me.pairs)
    print(f"{scene.name}: {lost} items lost to the mask")
    assert lost >= 6
    assert all(m.shape == unmasked.window.frames[i].pixelinfo.shape[:2] and 0 < (m == 0).sum() for i, m in enumerate(scene.masks))


@pytest.mark.parametrize("defect", sm.DEFECTS)
def test_defect_is_rejected(defect):
    """compare() must fail, on at least one scene, when the device's place is taken by the model's own central values computed with one
    deliberate mistake.  The states are the initial one (both sweeps) and the oracle's first step (residual-only sweep)."""
    rejected = []
    for name, builder in ses.F32_EDGE_SCENES:
        for fej in (1, 0):
            me, ml = _f32_results(builder, fej)
            de, dl = _f32_results(builder, fej, defect)
            fails, _ = sm.compare(sm.as_device(de, dl), me, ml)
            if not fails:
                m1, _ = _f32_results(builder, fej, stepped=True)
                d1, _ = _f32_results(builder, fej, defect, True)
                fails, _ = sm.compare(sm.as_device(d1), m1)
            if fails:
                rejected.append((name, fej, fails[0]))
    print(f"{defect}: rejected on {len(rejected)} of {2 * len(ses.F32_EDGE_SCENES)} (scene, fej) cases; first: {rejected[:1]}")
    assert rejected, defect
