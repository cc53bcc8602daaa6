"""Time of the device PnP RANSAC per call (dsopp_hip_pnp_ransac_estimate: pinned copy and upload of the matches and the sample triples, the
one launch that solves and scores every hypothesis, selects, refines the winner and selects again, the results' read-back, one wait), with
the library's configuration (256 hypotheses, threshold 0.5 px, 10 refinement iterations).  The object runs on a stream of torch's; device
time is taken with events on that stream around each call, host time with a clock around the call (it ends in the call's one wait).  Each
figure is the median of --calls calls after --warmup, on a 640 x 480 scene, f = 448, of points at 2 .. 10 m seen from the pose
exp((0.03, -0.05, 0.02)), t = (0.2, -0.1, 0.3), with 0.3 px of noise and 30 % outliers.  Prints one JSON line per point count.
    python scripts/time_pnp_ransac.py [--points 500,2000 --iterations 256 --calls 100 --warmup 10]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CAMERA = (448.0, 448.0, 320.0, 240.0, 640, 480)


def rotation(w):
    w = np.asarray(w, np.float64)
    t = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + np.sin(t) / t * K + (1 - np.cos(t)) / (t * t) * K @ K


def scene(n, seed):
    fx, fy, cx, cy, width, height = CAMERA
    rng = np.random.default_rng(seed)
    R, t = rotation([0.03, -0.05, 0.02]), np.array([0.2, -0.1, 0.3])
    px = np.stack([rng.uniform(8.0, width - 9.0, n), rng.uniform(8.0, height - 9.0, n)], axis=1)
    pc = np.stack([(px[:, 0] - cx) / fx, (px[:, 1] - cy) / fy, np.ones(n)], axis=1) * rng.uniform(2.0, 10.0, n)[:, None]
    X = (pc - t) @ R
    obs = px + rng.normal(0.0, 0.3, (n, 2))
    out = rng.random(n) < 0.3
    obs[out] += rng.normal(0.0, 15.0, (int(out.sum()), 2))
    samples = np.array([rng.choice(n, 3, replace=False) for _ in range(4096)], np.int32)
    return X, obs, samples


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="500,2000")
    ap.add_argument("--iterations", type=int, default=256)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    import torch  # the stream and its events are torch's (plumbing); its HIP runtime comes up before the library's
    from dsopp_amd import capi
    if not torch.cuda.is_available() or capi.device_count() < 1:
        raise SystemExit("time_pnp_ransac.py needs a GPU: dsopp_amd has no CPU fallback")
    torch.cuda.init()
    stream = torch.cuda.Stream()
    for n in (int(v) for v in args.points.split(",")):
        X, obs, pool = scene(n, 1)
        r = capi.PnpRansac(stream=stream.cuda_stream)
        dev, host, inliers, refined, its = [], [], [], [], []
        for k in range(args.warmup + args.calls):
            first = (k * args.iterations) % (len(pool) - args.iterations)
            samples = pool[first:first + args.iterations]  # other triples every call
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            t0 = time.perf_counter()
            got = r.estimate(CAMERA, X, obs, samples)
            t1 = time.perf_counter()
            e1.record(stream)
            e1.synchronize()
            if k >= args.warmup:
                dev.append(e0.elapsed_time(e1))
                host.append((t1 - t0) * 1e3)
                inliers.append(got["ransac_inlier_count"])
                refined.append(got["refined_inlier_count"])
                its.append(got["refine_iterations"])
        r.close()
        print(json.dumps({"points": n, "iterations": args.iterations, "calls": args.calls, "estimate_device_ms_median": float(np.median(dev)),
                          "estimate_device_ms_min_max": [float(np.min(dev)), float(np.max(dev))], "estimate_host_ms_median": float(np.median(host)),
                          "ransac_inliers_mean": float(np.mean(inliers)), "refined_inliers_mean": float(np.mean(refined)),
                          "refine_iterations_mean": float(np.mean(its))}), flush=True)


if __name__ == "__main__":
    main()
