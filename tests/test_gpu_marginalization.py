"""dsopp_hip_window_note_optimization / _choose_marginalization against tests/marginalization_model.py, which is given the state the
window itself reports (flags, n_inliers, inverse depths, 1 / H_dd, poses, statuses towards the newest keyframe, counters): selected set,
marginalised keyframes, counts and every flag byte exactly, the scores to 1e-10 relative — coordinates stay below 10 in magnitude and
pairwise distances above 1e-3, so a coordinate difference carries at most 2.2e-15 of absolute rounding, 2.2e-12 of the distance, and
fewer than 40 roundings follow.  Images are 64 x 48."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import marginalization_model as mm
from dsopp_amd import synthetic as syn

pytestmark = pytest.mark.gpu

W, H = 64, 48
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Scene:
    """a synthetic window cut to the landmark counts asked for, with seeded flags at upload, statuses, and immature landmarks"""

    def __init__(self, counts, seed, spare=0, small=(), short=None, random_poses=False, immature_on=()):
        F = len(counts)
        self.win = syn.make_window(num_frames=F + spare, num_points=(F + spare) * max(max(counts), 65), width=W, height=H, seed=seed)
        rng = np.random.default_rng(seed + 100)
        self.frames = self.win.frames[:F]
        self.spare = self.win.frames[F:]
        self.flags, self.statuses, self.immature = {}, {}, {}
        for k, (f, n) in enumerate(zip(self.frames, counts)):
            f.uv, f.idepth_gt, f.idepth_init, f.patch = f.uv[:n], f.idepth_gt[:n], f.idepth_init[:n], f.patch[:n]
            fl = (rng.random(n) < 0.1).astype(np.uint8) * rng.integers(1, 3, n).astype(np.uint8)
            if k in small:  # nearly everything gone: findFramesWithSmallNumberOfActivePoints takes the frame
                fl[:] = rng.integers(1, 4, n)
                fl[:2] = 0
            self.flags[f.frame_id] = fl
            if random_poses:  # no solve follows: any pose will do, coordinates up to 10
                T = syn.se3_exp(np.concatenate([rng.uniform(-1, 1, 3), rng.uniform(-0.3, 0.3, 3)]))
                T[:3, 3] = rng.uniform(-10, 10, 3)
                f.T_w_c_init = T
        for a in self.frames:
            for b in self.frames:
                if a.frame_id == b.frame_id:
                    continue
                st = np.zeros(len(a.uv), dtype=np.uint8)
                bad = rng.random(len(a.uv)) < 0.15
                st[bad] = rng.integers(1, 5, int(bad.sum()))
                if short is not None and (a.frame_id, b.frame_id) == short:
                    st = st[:len(st) // 2]  # one connection shorter than its frame
                self.statuses[(a.frame_id, b.frame_id)] = st
        for k in immature_on:
            n = 70 + 13 * k
            lms = syn.new_immature_landmarks(rng.uniform(8, 40, (n, 2)), np.ones((n, 3)), np.zeros((n, 8)), np.zeros((n, 2)))
            lms["status"] = rng.integers(0, 7, n).astype(np.uint8)
            lms["idepth_min"] = rng.uniform(-0.2, 0.3, n)
            lms["idepth_max"] = lms["idepth_min"] + rng.uniform(0, 0.4, n)
            lms["uniqueness"] = rng.uniform(1, 6, n)
            lms["search_pixel_interval"] = rng.uniform(0, 16, n)
            lms["traced"] = rng.integers(0, 2, n).astype(np.uint8)
            self.immature[self.frames[k].frame_id] = lms

    def load(self, w, two_batches=()):
        intr = self.win.scene.intrinsics
        for k, f in enumerate(self.frames):
            w.push_frame(f.frame_id, f.timestamp, f.pixelinfo, None, intr, syn.mat_to_params(f.T_w_c_init), f.exposure, f.affine_init, f.fixed, False)
            fl = self.flags[f.frame_id]
            if k in two_batches:  # the device sorts every batch on its own: internal and caller's order differ across the two
                h = len(f.uv) // 3
                w.set_landmarks(f.frame_id, f.uv[:h], f.idepth_init[:h], f.patch[:h], fl[:h])
            w.set_landmarks(f.frame_id, f.uv, f.idepth_init, f.patch, fl)
        for (r, t), st in self.statuses.items():
            if len(st):
                w.set_connection(r, t, st)
        return w

    def sets(self, capi):
        out = []
        for f in self.frames:
            lms = self.immature.get(f.frame_id)
            if lms is None:
                out.append(None)
                continue
            s = capi.ImmatureSet(lms)
            s.upload(lms)
            out.append(s)
        return out


def status_towards(w, capi, ref_id, tgt_id, n):
    st = np.zeros(n, dtype=np.uint8)
    if n:
        capi._chk(capi.lib().dsopp_hip_window_get_residuals(w._h, int(ref_id), int(tgt_id), n, st.ctypes.data_as(C.c_void_p), None, None))
    return st


def model_frames(w, capi, sc, camera_ids=None):
    """the active frames as the model takes them, from what the window reports"""
    ids = w.frame_ids()
    last = ids[-1]
    out = []
    for k, fid in enumerate(ids):
        lm = w.get_landmarks(fid, False)
        T, _ = w.get_pose(fid)
        status = None
        if fid != last and len(sc.statuses.get((fid, last), ())):
            status = status_towards(w, capi, fid, last, len(sc.statuses[(fid, last)]))
        out.append(dict(camera_id=int(camera_ids[k]) if camera_ids is not None else fid, t=T[4:7].copy(), flags=lm["flags"] & 3,
                        n_inliers=lm["n_inliers"], successes=w.get_optimization_counts(fid), idepth=lm["idepth"], variance=lm["inv_hdd"],
                        status_last=status, immature=sc.immature.get(fid)))
    return out


def check_against_model(got, want, ids):
    assert got["selected"] == want.selected
    assert got["marginalized_ids"] == [ids[a] for a in want.marginalized]
    assert got["n_active_landmarks"] == want.n_kept and got["n_marginalized_landmarks"] == want.n_gone
    for fid, flags in zip(ids, want.flags):
        assert np.array_equal(got["flags"][fid], flags), fid
    assert (got["n_newly_marginalized"], got["n_newly_outlier"]) == (want.n_newly_marginalized, want.n_newly_outlier)
    assert np.array_equal(np.isnan(got["scores"]), np.isnan(want.scores))
    ok = ~np.isnan(want.scores)
    print("scores", got["scores"], "model", want.scores)
    assert np.all(np.abs(got["scores"][ok] - want.scores[ok]) <= 1e-10 * np.abs(want.scores[ok]))
    best = np.sort(want.scores[ok])[::-1]
    if len(best) >= 2:  # the choice must not hang on the last bits
        assert best[0] - best[1] > 1e-6 * best[0], best[:2]


def options_of(capi, o):
    return capi.default_marginalization_options(strategy=o.strategy, minimum_size=o.minimum_size, maximum_size=o.maximum_size,
                                                maximum_share_marginalized=o.maximum_share_marginalized)


# landmark counts at wavefront and workgroup edges, and an empty frame; the options make both frame rules run where the window allows it
CASES = {
    "3_frames_no_solve": dict(counts=[257, 0, 65], seed=3, options=mm.Options(mm.SPARSE, 1, 2, 0.95), solve=False, short=(0, 2), two_batches=(0,),
                              immature_on=(0,), camera_ids=None),
    "5_frames": dict(counts=[64, 1, 257, 63, 65], seed=5, options=mm.Options(mm.SPARSE, 3, 4, 0.95), solve=True, short=(2, 4), two_batches=(2, 3),
                     immature_on=(0, 3), camera_ids=[7, 9, 30, 30, 30]),
    "8_frames": dict(counts=[65, 63, 257, 64, 1, 65, 0, 63], seed=8, options=mm.Options(mm.SPARSE, 5, 6, 0.95), solve=True, short=(3, 7),
                     two_batches=(0, 2), immature_on=(2, 5, 6), camera_ids=[100 + 3 * i for i in range(8)], small=(1,)),
}


def build(capi, case, deterministic=False, spare=0):
    c = CASES[case]
    sc = Scene(c["counts"], c["seed"], spare=spare, small=c.get("small", ()), short=c["short"], random_poses=not c["solve"], immature_on=c["immature_on"])
    w = capi.HipWindow(capi.default_pba_options())
    if deterministic:
        w.set_deterministic(True)
    sc.load(w, c["two_batches"])
    if c["solve"]:
        w.solve()
        for _ in range(2 * c["options"].maximum_size + 1):  # enough for numberOfSuccessfulOptimizations > 2 * maximum_size
            w.note_optimization()
    return sc, w


@pytest.mark.parametrize("case", list(CASES))
def test_decisions_match_the_model(case):
    from dsopp_amd import capi
    c = CASES[case]
    sc, w = build(capi, case)
    sets = sc.sets(capi)
    frames = model_frames(w, capi, sc, c["camera_ids"])
    want = mm.choose(frames, c["options"])
    before = {fid: w.get_landmarks(fid, False)["flags"] for fid in w.frame_ids()}
    got = w.choose_marginalization(options_of(capi, c["options"]), c["camera_ids"], sets, apply=False)
    ids = w.frame_ids()
    assert got["active_ids"] == ids
    check_against_model(got, want, ids)
    if c["solve"]:  # the solved windows reach every landmark rule
        assert want.n_newly_marginalized > 0 and want.n_newly_outlier > 0 and len(want.marginalized) >= 1
    if case == "8_frames":
        assert len(want.selected) == 2 and want.marginalized[1] == want.selected[1] + 1  # the shifted erase
    # apply = 0 changed nothing
    assert w.frame_ids() == ids
    for fid in ids:
        assert np.array_equal(w.get_landmarks(fid, False)["flags"], before[fid])
    # the same call again: the same bytes
    again = w.choose_marginalization(options_of(capi, c["options"]), c["camera_ids"], sets, apply=False)
    assert again["scores"].tobytes() == got["scores"].tobytes()
    assert all(again[k] == got[k] for k in got if k not in ("scores", "flags"))
    assert all(again["flags"][fid].tobytes() == got["flags"][fid].tobytes() for fid in ids)
    # without the immature sets the counts lose the landmarks ready for activation
    bare = w.choose_marginalization(options_of(capi, c["options"]), c["camera_ids"], None, apply=False)
    for f in frames:
        f["immature"] = None
    assert bare["n_active_landmarks"] == mm.choose(frames, c["options"]).n_kept
    assert sum(bare["n_active_landmarks"]) < sum(got["n_active_landmarks"])
    for s in sets:
        if s is not None:
            s.close()
    w.close()


@pytest.mark.parametrize("F", [3, 6])
def test_counter(F):
    """F frames of 65 landmarks, n_inliers of a real solve; landmarks appended between calls start at 0; earlier rows survive an append whose
    connection ends inside the new batch, which re-orders the frame on the device.  (A landmark of a 3-frame window has two residuals and
    never more than 3 inliers: its counters stay 0; the 6-frame window has both outcomes.)"""
    from dsopp_amd import capi
    win = syn.make_window(num_frames=F, num_points=F * 100, width=W, height=H, seed=11)
    full = {f.frame_id: (f.uv, f.idepth_init, f.patch) for f in win.frames}
    for f in win.frames:
        f.uv, f.idepth_gt, f.idepth_init, f.patch = f.uv[:65], f.idepth_gt[:65], f.idepth_init[:65], f.patch[:65]
    w = syn.load_window(capi.HipWindow(capi.default_pba_options()), win)
    ids = w.frame_ids()
    assert all(np.array_equal(w.get_optimization_counts(fid), np.zeros(65, np.int32)) for fid in ids)  # before the first note
    w.solve()
    want = {}
    for fid in ids:
        lm = w.get_landmarks(fid, False)
        want[fid] = mm.note_optimization(mm.note_optimization(np.zeros(65, np.int32), lm["flags"], lm["n_inliers"]), lm["flags"], lm["n_inliers"])
    if F > 4:
        assert sum(int(v.sum()) for v in want.values()) > 0 and any((v == 0).any() for v in want.values())  # both outcomes occur
    w.note_optimization()
    w.note_optimization()
    for fid in ids:
        assert np.array_equal(w.get_optimization_counts(fid), want[fid]), fid
    # 35 more landmarks for the middle frame; its connections end at 80, inside the new batch
    mid = ids[1]
    uv, idepth, patch = full[mid]
    w.set_landmarks(mid, uv, idepth, patch, np.zeros(100, dtype=np.uint8))
    for t in ids:
        if t != mid:
            w.set_connection(mid, t, np.zeros(80, dtype=np.uint8))
    assert np.array_equal(w.get_optimization_counts(mid), np.concatenate([want[mid], np.zeros(35, np.int32)]))
    w.note_optimization()
    for fid in ids:
        lm = w.get_landmarks(fid, False)
        start = np.concatenate([want[fid], np.zeros(len(lm["flags"]) - 65, np.int32)])
        assert np.array_equal(w.get_optimization_counts(fid), mm.note_optimization(start, lm["flags"], lm["n_inliers"])), fid
    assert np.array_equal(w.get_optimization_counts(mid)[65:], np.zeros(35, np.int32))  # never optimised: n_inliers is 0
    w.snapshot()
    w.note_optimization()
    after = {fid: w.get_optimization_counts(fid) for fid in ids}
    w.restore()
    assert all(np.array_equal(w.get_optimization_counts(fid), after[fid]) for fid in ids)  # the counters are no part of a snapshot
    w.close()


def test_apply_equals_the_flag_refresh_of_set_landmarks():
    """window A applies on the device, window B is given the model's flags through set_landmarks and mark_frame_marginalized: the same
    flags (to_marginalize included), and after the same push_frame the same frames and the same prior (1e-7, the bar of test_marginalization.py)"""
    from dsopp_amd import capi
    c = CASES["8_frames"]
    windows = []
    for _ in range(2):
        sc, w = build(capi, "8_frames", deterministic=True, spare=1)
        windows.append((sc, w))
    (sc, a), (_, b) = windows
    ids = a.frame_ids()
    want = mm.choose(model_frames(b, capi, sc, c["camera_ids"]), c["options"])
    sets = sc.sets(capi)
    got = a.choose_marginalization(options_of(capi, c["options"]), c["camera_ids"], sets, apply=True)
    check_against_model(got, want, ids)
    for f, flags in zip(sc.frames, want.flags):
        b.set_landmarks(f.frame_id, f.uv, f.idepth_init, f.patch, flags)
    for k in want.marginalized:
        b.mark_frame_marginalized(ids[k])
    n_pending = 0
    for fid in ids:
        fa, fb = a.get_landmarks(fid, False)["flags"], b.get_landmarks(fid, False)["flags"]
        assert np.array_equal(fa, fb), fid
        n_pending += int(np.count_nonzero(fa & 4))
    assert n_pending > 0  # landmarks wait for the fold-in
    # the frames flagged are no longer active
    assert a.choose_marginalization(options_of(capi, c["options"]), c["camera_ids"], sets, apply=False)["active_ids"] == \
        [fid for k, fid in enumerate(ids) if k not in want.marginalized]
    new = sc.spare[0]
    intr = sc.win.scene.intrinsics
    for w in (a, b):
        w.push_frame(new.frame_id, new.timestamp, new.pixelinfo, None, intr, syn.mat_to_params(new.T_w_c_init), new.exposure, new.affine_init, False, False)
    assert a.frame_ids() == b.frame_ids() == [fid for k, fid in enumerate(ids) if k not in want.marginalized] + [new.frame_id]
    (Ha, ba, ea), (Hb, bb, eb) = a.get_marginalized(), b.get_marginalized()
    assert Ha.shape == Hb.shape and np.abs(Hb).max() > 0
    assert np.abs(Ha - Hb).max() <= 1e-7 * np.abs(Hb).max()
    assert np.abs(ba - bb).max() <= 1e-7 * max(1.0, np.abs(bb).max())
    assert abs(ea - eb) <= 1e-7 * abs(eb)
    for s in sets:
        if s is not None:
            s.close()
    a.close()
    b.close()


def test_maximum_size_strategy():
    from dsopp_amd import capi
    sc = Scene([65, 64, 1, 63, 65, 0, 64, 65, 63], seed=9, random_poses=True)
    w = sc.load(capi.HipWindow(capi.default_pba_options()))
    ids = w.frame_ids()
    opts = mm.Options(mm.MAXIMUM_SIZE, 5, 7, 0.95)
    want = mm.choose(model_frames(w, capi, sc), opts)
    assert want.marginalized == [0, 1]
    got = w.choose_marginalization(options_of(capi, opts), apply=True)
    check_against_model(got, want, ids)
    assert got["marginalized_ids"] == ids[:2]
    for k, fid in enumerate(ids):
        flags = w.get_landmarks(fid, False)["flags"]
        assert np.array_equal(flags & 1, np.ones(len(flags), np.uint8) if k < 2 else sc.flags[fid] & 1)
    assert w.choose_marginalization(options_of(capi, opts))["active_ids"] == ids[2:]
    w.close()


def test_example_driver(tmp_path):
    """example_marginalization.cpp drives HipFrameMarginalizationStrategy over the C-ABI alone and checks its own choices"""
    from test_marginalization_model import build_example
    r = subprocess.run([build_example(tmp_path), "-v"], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
