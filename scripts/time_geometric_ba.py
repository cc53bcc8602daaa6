"""Time of the device geometric bundle adjustment per call (dsopp_hip_geometric_ba_solve, _triangulate and _flag_outliers: pinned copy and
upload of the problem, the launches, the read-back, the waits).  The object runs on a stream of torch's; device time is taken with events
on that stream around each call, host time with a clock around the call.  Each figure is the median of --calls calls after --warmup, on
the synthetic bootstrap scene of tests/geometric_ba_model.py (640 x 480, F frames, L landmarks seen in 2 .. F of them, 0.3 px of noise,
the state perturbed off the truth), with the reference's solver options.  solve is timed for every iteration-group size of --groups: the
number of iterations enqueued between two reads of the state record.  Prints one JSON line per landmark count.
    python scripts/time_geometric_ba.py [--frames 10 --landmarks 500,3000 --groups 1,2,4,8,16,50 --calls 100 --warmup 10]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--landmarks", default="500,3000")
    ap.add_argument("--groups", default="1,2,4,8,16,50")
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    import torch  # the stream and its events are torch's (plumbing); its HIP runtime comes up before the library's
    import geometric_ba_model as gm
    from dsopp_amd import capi
    if not torch.cuda.is_available() or capi.device_count() < 1:
        raise SystemExit("time_geometric_ba.py needs a GPU: dsopp_amd has no CPU fallback")
    torch.cuda.init()
    stream = torch.cuda.Stream()

    def timed(call):
        dev, host, last = [], [], None
        for k in range(args.warmup + args.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            t0 = time.perf_counter()
            last = call()
            t1 = time.perf_counter()
            e1.record(stream)
            e1.synchronize()
            if k >= args.warmup:
                dev.append(e0.elapsed_time(e1))
                host.append((t1 - t0) * 1e3)
        return {"device_ms_median": float(np.median(dev)), "device_ms_min_max": [float(np.min(dev)), float(np.max(dev))],
                "host_ms_median": float(np.median(host))}, last

    for L in (int(v) for v in args.landmarks.split(",")):
        truth, rng = gm.make_scene(F=args.frames, L=L, seed=8, noise=0.3)
        start = gm.perturb(truth, rng)
        problem = (start.cam, start.poses, start.X, start.off, start.ofr, start.oxy)
        b = capi.GeometricBA(stream=stream.cuda_stream)
        line = {"frames": args.frames, "landmarks": L, "observations": int(start.M), "calls": args.calls, "solve": {}}
        for group in (int(v) for v in args.groups.split(",")):
            figures, out = timed(lambda: b.solve(*problem, iteration_group=group))
            figures.update(iterations=out["iterations"], accepted=out["accepted_steps"], reason=out["reason"])
            line["solve"][str(group)] = figures
        has = np.zeros(L, np.uint8)
        line["triangulate"], (done, _) = timed(lambda: b.triangulate(*problem, has, 4, False))
        line["triangulated"] = int(done.sum())
        line["flag_outliers"], flags = timed(lambda: b.flag_outliers(truth.cam, truth.poses, truth.X, truth.off, truth.ofr, truth.oxy))
        line["flagged"] = int(flags.sum())
        b.close()
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
