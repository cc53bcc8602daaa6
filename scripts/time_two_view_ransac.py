"""Time of the device's two-view pose per call (dsopp_hip_two_view_ransac_estimate: pinned copy and upload of the matches and the samples,
the one launch that solves and scores every five-point hypothesis, selects, refines the winner, selects again and refines again, the
results' read-back, one wait), with the library's configuration (256 hypotheses, threshold 0.5 px, 40 refinement iterations at most), and
of the two-view triangulation of the same matches.  The object runs on a stream of torch's; device time is taken with events on that
stream around each call, host time with a clock around the call (it ends in the call's one wait).  Each figure is the median of --calls
calls after --warmup, on a 640 x 480 scene, f = 448, of points at 3 .. 12 baselines seen from two frames a rotation of
(0.04, -0.06, 0.03) and a unit translation along (0.9, -0.1, 0.4) apart, with 0.3 px of noise and 30 % outliers.  Prints one JSON line per
match count.
    python scripts/time_two_view_ransac.py [--matches 257,2000 --iterations 256 --calls 100 --warmup 10]"""
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
IDENTITY = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])


def rotation(w):
    w = np.asarray(w, np.float64)
    t = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + np.sin(t) / t * K + (1 - np.cos(t)) / (t * t) * K @ K


def scene(n, seed):
    fx, fy, cx, cy, width, height = CAMERA
    rng = np.random.default_rng(seed)
    R, t = rotation([0.04, -0.06, 0.03]), np.array([0.9, -0.1, 0.4]) / np.linalg.norm([0.9, -0.1, 0.4])
    A = np.zeros((0, 2))
    B = np.zeros((0, 2))
    while len(A) < n:
        a = np.stack([rng.uniform(8.0, width - 9.0, n), rng.uniform(8.0, height - 9.0, n)], axis=1)
        pa = np.stack([(a[:, 0] - cx) / fx, (a[:, 1] - cy) / fy, np.ones(n)], axis=1) * rng.uniform(3.0, 12.0, n)[:, None]
        pb = (pa - t) @ R                                  # R^T (p - t), per row
        b = np.stack([fx * pb[:, 0] / pb[:, 2] + cx, fy * pb[:, 1] / pb[:, 2] + cy], axis=1)
        seen = (pb[:, 2] > 0.5) & (b[:, 0] >= 8.0) & (b[:, 0] <= width - 9.0) & (b[:, 1] >= 8.0) & (b[:, 1] <= height - 9.0)
        A, B = np.vstack([A, a[seen]]), np.vstack([B, b[seen]])
    A, B = A[:n] + rng.normal(0.0, 0.3, (n, 2)), B[:n] + rng.normal(0.0, 0.3, (n, 2))
    out = rng.random(n) < 0.3
    B[out] += rng.normal(0.0, 15.0, (int(out.sum()), 2))
    samples = np.array([rng.choice(n, 5, replace=False) for _ in range(4096)], np.int32)
    return A, B, samples


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matches", default="257,2000")
    ap.add_argument("--iterations", type=int, default=256)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    import torch  # the stream and its events are torch's (plumbing); its HIP runtime comes up before the library's
    from dsopp_amd import capi
    if not torch.cuda.is_available() or capi.device_count() < 1:
        raise SystemExit("time_two_view_ransac.py needs a GPU: dsopp_amd has no CPU fallback")
    torch.cuda.init()
    stream = torch.cuda.Stream()
    for n in (int(v) for v in args.matches.split(",")):
        A, B, pool = scene(n, 1)
        r = capi.TwoViewRansac(stream=stream.cuda_stream)
        dev, host, tri, ransac, inliers, its, solutions = [], [], [], [], [], [], []
        for k in range(args.warmup + args.calls):
            first = (k * args.iterations) % (len(pool) - args.iterations)
            samples = pool[first:first + args.iterations]  # other samples every call
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record(stream)
            t0 = time.perf_counter()
            got = r.estimate(CAMERA, A, B, samples)
            t1 = time.perf_counter()
            e1.record(stream)
            _, keep = r.triangulate(CAMERA, A, B, got["pose"], IDENTITY)
            e2.record(stream)
            e2.synchronize()
            if k >= args.warmup:
                dev.append(e0.elapsed_time(e1))
                tri.append(e1.elapsed_time(e2))
                host.append((t1 - t0) * 1e3)
                ransac.append(got["ransac_inlier_count"])
                inliers.append(got["inlier_count"])
                its.append(sum(got["refine_iterations"]))
                solutions.append(int(keep.sum()))
        r.close()
        print(json.dumps({"matches": n, "iterations": args.iterations, "calls": args.calls, "estimate_device_ms_median": float(np.median(dev)),
                          "estimate_device_ms_min_max": [float(np.min(dev)), float(np.max(dev))], "estimate_host_ms_median": float(np.median(host)),
                          "triangulate_device_ms_median": float(np.median(tri)), "ransac_inliers_mean": float(np.mean(ransac)),
                          "inliers_mean": float(np.mean(inliers)), "refine_iterations_mean": float(np.mean(its)),
                          "triangulated_mean": float(np.mean(solutions))}), flush=True)


if __name__ == "__main__":
    main()
