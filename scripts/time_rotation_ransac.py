"""Time of the device rotation RANSAC per call (dsopp_hip_rotation_ransac_estimate: pinned copy and upload of the pairs and the sample
triples, the one launch that scores every hypothesis and selects, the results' read-back, one wait), with the reference's configuration
(200 iterations, threshold 1.5 px, tolerance 0.95).  The object runs on a stream of torch's; device time is taken with events on that
stream around each call, host time with a clock around the call (it ends in the call's one wait).  Each figure is the median of --calls
calls after --warmup, on a 640 x 480 scene rotated by exp((0.01, -0.02, 0.005)) with 0.4 px of noise and 30 % outliers.  Prints one
JSON line per point count.
    python scripts/time_rotation_ransac.py [--points 500,2000 --iterations 200 --calls 100 --warmup 10]"""
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
    A = np.stack([rng.uniform(4.0, width - 5.0, n), rng.uniform(4.0, height - 5.0, n)], axis=1)
    u = np.stack([(A[:, 0] - cx) / fx, (A[:, 1] - cy) / fy, np.ones(n)], axis=1) @ rotation([0.01, -0.02, 0.005]).T
    B = np.stack([fx * u[:, 0] / u[:, 2] + cx, fy * u[:, 1] / u[:, 2] + cy], axis=1) + rng.normal(0.0, 0.4, (n, 2))
    out = rng.random(n) < 0.3
    B[out] += rng.normal(0.0, 15.0, (int(out.sum()), 2))
    samples = np.array([rng.choice(n, 3, replace=False) for _ in range(4096)], np.int32)
    return A, B, samples


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="500,2000")
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    import torch  # the stream and its events are torch's (plumbing); its HIP runtime comes up before the library's
    from dsopp_amd import capi
    if not torch.cuda.is_available() or capi.device_count() < 1:
        raise SystemExit("time_rotation_ransac.py needs a GPU: dsopp_amd has no CPU fallback")
    torch.cuda.init()
    stream = torch.cuda.Stream()
    for n in (int(v) for v in args.points.split(",")):
        A, B, pool = scene(n, 1)
        r = capi.RotationRansac(stream=stream.cuda_stream)
        dev, host, inliers, run = [], [], [], []
        for k in range(args.warmup + args.calls):
            first = (k * args.iterations) % (len(pool) - args.iterations)
            samples = pool[first:first + args.iterations]  # other triples every call
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            t0 = time.perf_counter()
            got = r.estimate(CAMERA, A, B, samples)
            t1 = time.perf_counter()
            e1.record(stream)
            e1.synchronize()
            if k >= args.warmup:
                dev.append(e0.elapsed_time(e1))
                host.append((t1 - t0) * 1e3)
                inliers.append(got["inlier_count"])
                run.append(got["iterations_run"])
        r.close()
        print(json.dumps({"points": n, "iterations": args.iterations, "calls": args.calls, "estimate_device_ms_median": float(np.median(dev)),
                          "estimate_device_ms_min_max": [float(np.min(dev)), float(np.max(dev))], "estimate_host_ms_median": float(np.median(host)),
                          "inliers_mean": float(np.mean(inliers)), "iterations_run_mean": float(np.mean(run))}), flush=True)


if __name__ == "__main__":
    main()
