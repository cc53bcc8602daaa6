"""Time of the device optical-flow tracker per call, with the reference's configuration (window 15, 3 pyramid levels below the image, 10
iterations, epsilon 0.01): dsopp_hip_flow_tracker_set_reference (pinned copy, upload, the levels and Scharr planes of image_from) and
dsopp_hip_flow_tracker_track (pinned copy, upload, the levels of image_to, the tracking launch, the results' read-back).  The tracker
runs on a stream of torch's; device time is taken with events on that stream around each call, host time with a clock around the call
(track ends in a synchronise; set_reference only enqueues, so its host time is the enqueue).  Each figure is the median of --calls calls
after --warmup, on a textured image shifted by a few pixels between the frames.  Prints one JSON line per size.
    python scripts/time_optical_flow.py [--sizes 640x480,1280x1024 --points 2000 --calls 100 --warmup 10]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def texture(width, height, shift):
    y, x = np.mgrid[0:height, 0:width].astype(np.float64)
    x, y = x - shift[0], y - shift[1]
    v = (128.0 + 34.0 * np.sin(0.110 * x + 0.070 * y) + 30.0 * np.sin(0.050 * x - 0.130 * y + 1.0) + 26.0 * np.sin(0.170 * x + 0.150 * y + 2.0) +
         22.0 * np.cos(0.230 * x - 0.040 * y + 0.5) + 12.0 * np.sin(0.031 * x + 0.220 * y))
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="640x480,1280x1024")
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    import torch  # the stream and its events are torch's (plumbing); its HIP runtime comes up before the library's
    from dsopp_amd import capi
    if not torch.cuda.is_available() or capi.device_count() < 1:
        raise SystemExit("time_optical_flow.py needs a GPU: dsopp_amd has no CPU fallback")
    torch.cuda.init()
    stream = torch.cuda.Stream()
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        frames = [texture(W, H, (1.3 * i, -0.9 * i)) for i in range(4)]
        rng = np.random.default_rng(1)
        pts = np.stack([rng.uniform(30, W - 30, args.points), rng.uniform(30, H - 30, args.points)], axis=1).astype(np.float32)
        t = capi.OpticalFlowTracker(W, H, stream=stream.cuda_stream)
        dev = {"set_reference": [], "track": []}
        host = {"set_reference": [], "track": []}
        tracked, passes = [], []
        for k in range(args.warmup + args.calls):
            for what in ("set_reference", "track"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                t0 = time.perf_counter()
                if what == "set_reference":
                    t.set_reference(frames[0])
                else:
                    to, status, err, iters = t.track(frames[1 + k % 3], pts, with_iterations=True)
                t1 = time.perf_counter()
                e1.record(stream)
                e1.synchronize()
                if k >= args.warmup:
                    dev[what].append(e0.elapsed_time(e1))
                    host[what].append((t1 - t0) * 1e3)
            if k >= args.warmup:
                tracked.append(int(status.sum()))
                passes.append(float(iters.sum(axis=1).mean()))
        t.close()
        out = {"size": size, "points": args.points, "levels": t.num_levels, "calls": args.calls}
        for what in ("set_reference", "track"):
            out[f"{what}_device_ms_median"] = float(np.median(dev[what]))
            out[f"{what}_device_ms_min_max"] = [float(np.min(dev[what])), float(np.max(dev[what]))]
            out[f"{what}_host_ms_median"] = float(np.median(host[what]))
        out["tracked_mean"] = float(np.mean(tracked))
        out["passes_per_point_mean"] = float(np.mean(passes))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
