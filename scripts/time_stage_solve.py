"""Device time of the stage API's solve launch (assembleSolveKernel with do_solve: calculate_step, every step of lm_mode 1), per launch,
from the window's own profile (a HIP event pair around every launch).  One JSON line per window: the C1 window (7 keyframes, 2000
points, 640 x 480) and the 2-, 8- and 9-keyframe case windows of tests/dense_solve_model.py (9: the K > 64 path).

    python scripts/time_stage_solve.py [label] [calls]      # DSOPP_HIP_LIB selects the library"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import dense_solve_model as dm
from dsopp_amd import capi, synthetic as syn

label = sys.argv[1] if len(sys.argv) > 1 else ""
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 300
windows = [("c1_7kf_2000", syn.make_window(7, 2000, 640, 480, seed=0))] + [(f"case_{F}kf", dm.make_case_window(F)) for F in (2, 8, 9)]
for name, win in windows:
    g = syn.load_window(capi.HipWindow(capi.default_pba_options()), win)
    lam = 1.0 / g.options.initial_trust_region_radius
    g.begin()
    g.calculate_energy()
    g.linearize()
    for _ in range(30):
        g.calculate_step(lam)
    g.set_profiling(True)
    for _ in range(calls):
        g.calculate_step(lam)
    ms, n = g.get_profile()["assemble_solve"]
    g.close()
    print(json.dumps({"build": label, "window": name, "launches": int(n), "assemble_solve_us_per_launch": round(1000.0 * ms / n, 3)}))
