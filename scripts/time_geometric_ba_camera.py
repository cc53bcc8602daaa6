"""Time per LM iteration of the geometric bundle adjustment on F10_L3000: the old entry point, solve_camera all fixed, solve_camera all free (pinhole and simple radial).
Host clock around the blocking call (it ends in an event synchronise); the variants alternate within every round; the per-iteration
figure is (t(50 iterations) - t(10 iterations)) / 40, which drops the call's upload, first linearisation and read-back."""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import geometric_ba_camera_model as gc
import test_gpu_geometric_ba_camera as t
from dsopp_amd import capi

ba = capi.GeometricBA()
pin, _, c_pin = t.camera_scene("F10_L3000", gc.PINHOLE)
rad, _, c_rad = t.camera_scene("F10_L3000", gc.SIMPLE_RADIAL)
kw = dict(function_tolerance=0.0, parameter_tolerance=0.0)
variants = {
    "old entry point": lambda n: ba.solve(*t.base.args(pin), max_iterations=n, **kw),
    "solve_camera, pinhole, all fixed": lambda n: ba.solve_camera(t.size(pin), gc.PINHOLE, pin.cam[:4], *t.state(pin), fixed=7, max_iterations=n, **kw),
    "solve_camera, pinhole, all free": lambda n: ba.solve_camera(t.size(pin), gc.PINHOLE, c_pin, *t.state(pin), max_iterations=n, **kw),
    "solve_camera, simple radial, all free": lambda n: ba.solve_camera(t.size(rad), gc.SIMPLE_RADIAL, c_rad, *t.state(rad), max_iterations=n, **kw),
}
times = {k: {10: [], 50: []} for k in variants}
info = {}
for rnd in range(3 + 60):
    for name, fn in variants.items():
        for n in (10, 50):
            t0 = time.perf_counter()
            out = fn(n)
            dt = time.perf_counter() - t0
            assert out["iterations"] == n, (name, out["iterations"])
            if rnd >= 3:
                times[name][n].append(dt)
            info[(name, n)] = (out["iterations"], out["accepted_steps"])
lines = []
for name in variants:
    a, b = np.array(times[name][10]), np.array(times[name][50])
    per = (b - a) / 40 * 1e6
    q = np.percentile(per, [25, 50, 75])
    lines.append(f"{name}: per LM iteration median {q[1]:.1f} us (quartiles {q[0]:.1f} .. {q[2]:.1f}, min {per.min():.1f}, max {per.max():.1f}); "
                 f"call of 50 iterations median {np.median(b) * 1e3:.3f} ms, of 10 {np.median(a) * 1e3:.3f} ms; accepted of 50: {info[(name, 50)][1]}")
print("\n".join(lines))
