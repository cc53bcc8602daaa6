"""The NumPy statement of updatePointStatuses (reference: src/energy/problems/src/photometric_bundle_adjustment.cpp:321-406): which residual
energies enter the third-quartile select, the threshold, which residuals become outliers, and what every landmark reports afterwards
(inlier count, relative baseline, the outlier bit).  Everything but one max of products is integer or a comparison of stored doubles, so
the model's statuses, energies, counts and flags are exact.  tests/test_point_status_model.py pins it on the CPU oracle,
tests/test_gpu_point_statuses.py holds the device to it.

Tables are in the layout the window API hands out: `residuals[(r, t)]` is get_residuals(r, t) (arrays `status`, `energy`) for every ordered
pair of frame ids that has a connection, `landmarks[r]` is get_landmarks(r) (`idepth`, `relative_baseline`, `flags`, `n_inliers`),
`marginalized[r]` the frame's marginalised bit, `centres[r]` the camera centre of its current pose."""
from collections import namedtuple

import numpy as np

from oracle import spec

OK, OUTLIER, OCCLUDED, OOB = 0, 1, 2, 3      # track::PointConnectionStatus as the window API encodes it
FLAG_MARGINALIZED, FLAG_OUTLIER = 1, 2
MIN_VALID_REPROJECTIONS = 1                   # minimum_valid_reprojections_num of solve()
EPS = np.finfo(np.float64).eps
# relative baseline: the distance from the model's value is held to BASELINE_FACTOR * eps * idepth * (|c_r| + |c_t|).  64 covers the
# subtraction's cancellation and the few roundings of the exponential map; the CPU oracle stays within 1.4239 of these units
# (tests/test_point_status_model.py, sigma 3 / seed 5; 0.9952 at sigma 20 / seed 4), so the bar is four times that
BASELINE_FACTOR = 5.7

# threshold: the energy above which a residual becomes an outlier (0 when nothing entered the select); n_select / rank / selected: how many
# energies entered, the 0-based rank taken and the energy found there (None when n_select = 0); residuals / landmarks: the expected tables;
# baseline_bound[r]: per landmark, how far an implementation's relative baseline may lie from the model's (relative_baseline_bound);
# n_outliers: residuals that were OK and are OUTLIER now
Result = namedtuple("Result", "threshold n_select rank selected residuals landmarks baseline_bound n_outliers")


def select_energies(ids, residuals, landmarks, marginalized):
    """the energies entering the select (:328-356): status OK, landmark not marginalised, target frame not marginalised, r != t"""
    out = []
    for r in ids:
        flags = np.asarray(landmarks[r]["flags"])
        for t in ids:
            if t == r or marginalized[t] or (r, t) not in residuals:
                continue
            res = residuals[(r, t)]
            m = len(res["status"])            # a residual list may be shorter than the landmark list (:347)
            take = (np.asarray(res["status"]) == OK) & ((flags[:m] & FLAG_MARGINALIZED) == 0)
            out.append(np.asarray(res["energy"], dtype=np.float64)[take])
    return np.concatenate(out) if out else np.zeros(0)


def relative_baseline_bound(idepth, old, norm_sum, is_old, factor):
    """factor * eps * idepth * (|c_r| + |c_t|): the subtraction c_r - c_t carries the rounding of both centres (cancellation), the norm and
    the product a few more; where the maximum is the previous value an equal term in it"""
    return factor * EPS * (np.abs(idepth) * norm_sum + np.where(is_old, np.abs(old), 0.0))


def update_point_statuses(ids, residuals, landmarks, marginalized, centres, sigma, baseline_factor=BASELINE_FACTOR):
    energies = select_energies(ids, residuals, landmarks, marginalized)
    n = int(energies.size)
    threshold = spec.third_quartile_threshold(energies, sigma)      # rank int(n * 0.75), selected + sigma^2 / 2 in double; 0.0 for n = 0
    rank = int(n * 0.75)
    selected = float(np.sort(energies)[rank]) if n else None
    out_res = {k: dict(status=np.array(v["status"], dtype=np.uint8), energy=np.array(v["energy"], dtype=np.float64)) for k, v in residuals.items()}
    out_lm, bounds = {}, {}
    n_outliers = 0
    for r in ids:
        lm = landmarks[r]
        flags = np.array(lm["flags"], dtype=np.uint8)
        idepth = np.asarray(lm["idepth"], dtype=np.float64)
        old = np.asarray(lm["relative_baseline"], dtype=np.float64)
        n_lm = len(flags)
        live = (flags & FLAG_MARGINALIZED) == 0                      # a marginalised landmark is skipped entirely (:373)
        inliers = np.zeros(n_lm, dtype=np.int64)
        baseline = old.copy()
        norm_sum = np.zeros(n_lm)                                    # largest |c_r| + |c_t| among the landmark's OK pairs
        for t in ids:
            if t == r or marginalized[t] or (r, t) not in residuals:
                continue
            res = out_res[(r, t)]
            m = len(res["status"])
            hit = live[:m] & (res["energy"] > threshold)              # whatever the status was: a fresh {kOutlier} residual (:389-391)
            n_outliers += int((hit & (res["status"] == OK)).sum())
            res["status"][hit] = OUTLIER
            res["energy"][hit] = 0.0
            ok = live[:m] & (res["status"] == OK)
            c_r, c_t = np.asarray(centres[r], dtype=np.float64), np.asarray(centres[t], dtype=np.float64)
            d = c_r - c_t
            distance = float(np.sqrt(np.sum(np.square(d.astype(np.longdouble)))))   # one rounding: the model adds no error of its own
            cand = idepth[:m] * distance
            baseline[:m] = np.where(ok, np.maximum(baseline[:m], cand), baseline[:m])
            # the error of a maximum is at most the largest error among its candidates: every OK pair counts towards the bound
            norm_sum[:m] = np.where(ok, np.maximum(norm_sum[:m], np.linalg.norm(c_r) + np.linalg.norm(c_t)), norm_sum[:m])
            inliers[:m] += ok
        before = np.asarray(lm.get("n_inliers", np.zeros(n_lm)), dtype=np.int64)
        new_flags = flags | np.where(live & (inliers < MIN_VALID_REPROJECTIONS), FLAG_OUTLIER, 0).astype(np.uint8)   # set, never cleared (:398-400)
        out_lm[r] = dict(n_inliers=np.where(live, inliers, before), relative_baseline=np.where(live, baseline, old), flags=new_flags)
        bounds[r] = np.where(live, relative_baseline_bound(idepth, old, norm_sum, baseline == old, baseline_factor), 0.0)
    return Result(threshold, n, rank, selected, out_res, out_lm, bounds, n_outliers)


def sharpness(energies, rank, sigma):
    """(selected - (predecessor + sigma^2 / 2), successor - (selected + sigma^2 / 2)) in sorted order; +inf where there is no neighbour.
    Both positive: a select that is one rank off in either direction moves the threshold across at least one energy (one rank low: the
    selected energy itself becomes an outlier; one rank high: the successor stays), and a status flips."""
    e = np.sort(np.asarray(energies, dtype=np.float64))
    below = e[rank] - (e[rank - 1] + sigma * sigma / 2) if rank > 0 else np.inf
    above = e[rank + 1] - (e[rank] + sigma * sigma / 2) if rank + 1 < len(e) else np.inf
    return float(below), float(above)


# ---------------------------------------------------------------------------------------------------------------------
# what both test files do around the rule: a window with an upper tail, reading the tables, holding a backend to the model
# ---------------------------------------------------------------------------------------------------------------------
def corrupt(win, seed):
    """the recipe of tests/test_oracle_statuses.py: a sixth of each frame's patches shifted by 25..90 grey levels, so that the energies have an
    upper tail and some landmarks lose every residual.  Returns the generator, for what a caller draws on top."""
    rng = np.random.default_rng(seed)
    for f in win.frames:
        bad = rng.choice(len(f.uv), len(f.uv) // 6, replace=False)
        f.patch[bad] += rng.uniform(25, 90, (len(bad), 1))
    return rng


def presets(win, rng):
    """on top of corrupt(): a tenth of the landmarks flagged marginalised and a few flagged outlier at upload, a share of the connections
    preset to OUTLIER / OCCLUDED / OOB.  Returns (statuses per ordered pair, flags per frame)."""
    statuses, flags = {}, {}
    for a in win.frames:
        n = len(a.uv)
        fl = np.zeros(n, dtype=np.uint8)
        fl[rng.choice(n, n // 10, replace=False)] = FLAG_MARGINALIZED
        fl[rng.choice(n, max(1, n // 40), replace=False)] |= FLAG_OUTLIER
        flags[a.frame_id] = fl
        for b in win.frames:
            if a.frame_id != b.frame_id:
                st = np.zeros(n, dtype=np.uint8)
                bad = rng.random(n) < 0.15
                st[bad] = rng.integers(1, 4, int(bad.sum()))
                statuses[(a.frame_id, b.frame_id)] = st
    return statuses, flags


def load(backend, win, statuses=None, flags=None):
    """dsopp_amd.synthetic.load_window with per-connection statuses and per-frame landmark flags"""
    from dsopp_amd import synthetic as syn
    intr = win.scene.intrinsics
    for i, f in enumerate(win.frames):
        backend.push_frame(f.frame_id, f.timestamp, f.pixelinfo, None, intr, syn.mat_to_params(f.T_w_c_init), f.exposure, f.affine_init, f.fixed, False)
        backend.set_landmarks(f.frame_id, f.uv, f.idepth_init, f.patch, np.zeros(len(f.uv), dtype=np.uint8) if flags is None else flags[f.frame_id])
        for g in win.frames[:i]:
            for (r, t) in ((g, f), (f, g)):
                st = None if statuses is None else statuses.get((r.frame_id, t.frame_id))
                backend.set_connection(r.frame_id, t.frame_id, np.zeros(len(r.uv), dtype=np.uint8) if st is None else st)
    return backend


def read_tables(backend, ids):
    """(residuals, landmarks, centres) as update_point_statuses takes them; pairs whose reference frame has no landmark are left out"""
    landmarks = {r: {k: v.copy() for k, v in backend.get_landmarks(r, False).items() if k in ("idepth", "relative_baseline", "flags", "n_inliers")}
                 for r in ids}
    residuals = {}
    for r in ids:
        for t in ids:
            if r != t and len(landmarks[r]["flags"]):
                res = backend.get_residuals(r, t)
                residuals[(r, t)] = dict(status=res["status"].copy(), energy=res["energy"].copy())
    centres = {r: backend.get_pose(r)[0][4:7].copy() for r in ids}
    return residuals, landmarks, centres


def mismatches(want, residuals, landmarks):
    """what of a backend's tables after the call differs from the model's Result: a list of strings, empty when all is as the rule says;
    and the largest relative-baseline difference in units of its bound"""
    bad, worst = [], 0.0
    for key, w in want.residuals.items():
        got = residuals[key]
        if not np.array_equal(got["status"], w["status"]):
            at = np.nonzero(got["status"] != w["status"])[0]
            bad.append(f"status {key}: {len(at)} differ, first at {at[0]}: got {got['status'][at[0]]} want {w['status'][at[0]]}")
        if not np.array_equal(got["energy"], w["energy"]):
            bad.append(f"energy {key}: {int((got['energy'] != w['energy']).sum())} differ")
    for r, w in want.landmarks.items():
        got = landmarks[r]
        if not np.array_equal(got["n_inliers"], w["n_inliers"]):
            bad.append(f"n_inliers of frame {r}: {int((got['n_inliers'] != w['n_inliers']).sum())} differ")
        if not np.array_equal(got["flags"], w["flags"]):
            bad.append(f"flags of frame {r}: {int((got['flags'] != w['flags']).sum())} differ")
        err, bound = np.abs(got["relative_baseline"] - w["relative_baseline"]), want.baseline_bound[r]
        if np.any(err > bound):
            i = int(np.argmax(err - bound))
            bad.append(f"relative_baseline of frame {r}: landmark {i} off by {err[i]:.3e}, bound {bound[i]:.3e}")
        if np.any((err > 0) & (bound > 0)):
            worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0])))
    return bad, worst
