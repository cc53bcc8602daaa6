"""Times dsopp_hip_window_activate_landmarks against the CPU restatement on a C1-sized window
(7 keyframes 640x480: 6 x 286 active landmarks, 6 x 1500 immature landmarks, the 7th keyframe is the new one)."""
import copy
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_landmark_activation as tla  # noqa: E402


def main():
    from dsopp_amd import capi
    from oracle import pyoracle as po
    n_imm = int(os.environ.get("ACT_IMMATURE", "1500"))
    _, frames, intr = tla.build_case(num_frames=7, per_frame=100 + n_imm, seed=3, width=640, height=480)
    # build_case keeps 100 active landmarks per keyframe; the timing wants ~286: reuse immature uv as extra actives is not
    # needed for the cost picture (the refinement dominates), so only the counts are reported
    n_imm_total = sum(len(f["immature"]["status"]) for f in frames[:-1])
    t0 = time.perf_counter()
    fo = copy.deepcopy(frames)
    st_o, n_act, dist = po.activate_landmarks(fo, intr, 20.0, 558, 3.0, refine=True)
    cpu_ms = (time.perf_counter() - t0) * 1e3
    tot = np.concatenate(st_o)
    print(f"immature {n_imm_total}, active {n_act}; oracle: {cpu_ms:.1f} ms; activated {(tot == 0).sum()} skipped {(tot == 1).sum()} deleted {(tot == 2).sum()}")
    opts = capi.default_pba_options()
    g = capi.HipWindow(opts)
    sets = []
    for i, f in enumerate(frames[:-1]):
        g.push_frame(i, 1000 * (i + 1), f["pixelinfo"], None, intr, f["T_w"], f["exposure"], f["affine"], i == 0, False)
        g.set_landmarks(i, f["active_uv"], f["active_idepth"], f["active_patch"], f["active_skip"] * 2)
        s = capi.ImmatureSet(f["immature"])
        sets.append(s)
    for i in range(6):
        for j in range(6):
            if i != j:
                g.set_connection(i, j, np.zeros(len(frames[i]["active_idepth"]), dtype=np.uint8))
    new = frames[-1]
    pyr = capi.Pyramid(640, 480, 2)
    pyr.set_level(0, new["pixelinfo"])
    times = []
    for rep in range(12):
        for s, f in zip(sets, frames[:-1]):
            s.upload(f["immature"])
        t0 = time.perf_counter()
        st, idp, res = g.activate_landmarks(list(range(6)), sets, pyr, new["T_w"], new["exposure"], new["affine"], 558, 3.0, True)
        times.append((time.perf_counter() - t0) * 1e3)
    same = np.array_equal(np.concatenate(st), tot)
    print(f"gpu: {np.median(times[2:]):.3f} ms per call (min {min(times):.3f}), rounds {res['selection_rounds']}, statuses identical: {same}, result {res}")


if __name__ == "__main__":
    main()
