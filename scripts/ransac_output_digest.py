"""SHA-256 of every output of the bootstrap's three RANSAC estimators and of the two-view triangulation on fixed seeded scenes: two builds
of the library compute the same bits exactly when this prints the same lines (DSOPP_HIP_LIB selects the build).  The scenes are the ones
of scripts/time_{rotation,pnp,two_view}_ransac.py; the shapes are the wave and workgroup edges and grids of one workgroup and of many,
not the workload's.  The per-hypothesis arrays are included; an inlier list is cut to its reported count.  Needs a GPU.
    python scripts/ransac_output_digest.py [--points 5,63,64,65,257,1000 --iterations 1,4,5,256]"""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "scripts")):
    if path not in sys.path:
        sys.path.insert(0, path)

import time_pnp_ransac as pnp  # noqa: E402
import time_rotation_ransac as rot  # noqa: E402
import time_two_view_ransac as tv  # noqa: E402


def report(unit, n, m, outputs):
    for name in sorted(outputs):
        a = np.ascontiguousarray(outputs[name])
        digest = hashlib.sha256(str((a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()
        print(f"{unit} n={n} iterations={m} {name} {digest}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="5,63,64,65,257,1000")
    ap.add_argument("--iterations", default="1,4,5,256")
    args = ap.parse_args()
    from dsopp_amd import capi
    if capi.device_count() < 1:
        raise SystemExit("ransac_output_digest.py needs a GPU: dsopp_amd has no CPU fallback")
    rotation, pose, two_view = capi.RotationRansac(), capi.PnpRansac(), capi.TwoViewRansac()
    for n in (int(v) for v in args.points.split(",")):
        scenes = rot.scene(n, 1), pnp.scene(n, 1), tv.scene(n, 1)
        for m in (int(v) for v in args.iterations.split(",")):
            A, B, pool = scenes[0]
            report("rotation", n, m, rotation.estimate(rot.CAMERA, A, B, pool[:m], with_hypotheses=True))
            X, obs, pool = scenes[1]
            report("pnp", n, m, pose.estimate(pnp.CAMERA, X, obs, pool[:m], with_hypotheses=True))
            A, B, pool = scenes[2]
            got = two_view.estimate(tv.CAMERA, A, B, pool[:m], min_matches=0, with_hypotheses=True)
            report("two_view", n, m, got)
            positions, keep = two_view.triangulate(tv.CAMERA, A, B, got["pose"], tv.IDENTITY)
            report("triangulate", n, m, {"positions": positions, "keep": keep})
    for handle in (rotation, pose, two_view):
        handle.close()


if __name__ == "__main__":
    main()
