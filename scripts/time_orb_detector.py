"""Time of the device ORB keypoint detector per call, with the reference's constants (500 features, 5 levels, edge threshold 31, FAST
threshold 20): dsopp_hip_orb_detector_detect_from_pyramid (the strided copy of the image a pyramid keeps, the level images, the FAST
score planes, suppression and histograms, the two cuts with the Harris responses between them, the results' read-back) and, beside it,
dsopp_hip_orb_detector_detect of a host image (the pinned copy and the upload in front of the same).  The detector and the pyramid run on
a stream of torch's; device time is taken with events on that stream around each call, host time with a clock around the call (both
calls end in a synchronise).  Each figure is the median of --calls calls after --warmup, on a texture of random 16-pixel cells with noise
of +-6, on which both cuts bite.  Prints one JSON line per size.
    python scripts/time_orb_detector.py [--sizes 640x480,1280x1024 --calls 100 --warmup 10]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def texture(width, height, seed, cell=16):
    rng = np.random.default_rng(seed)
    cells = rng.integers(0, 256, ((height + cell - 1) // cell, (width + cell - 1) // cell))
    img = np.kron(cells, np.ones((cell, cell), np.int64))[:height, :width] + rng.integers(-6, 7, (height, width))
    return np.clip(img, 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="640x480,1280x1024")
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    import torch  # the stream and its events are torch's (plumbing); its HIP runtime comes up before the library's
    from dsopp_amd import capi
    if not torch.cuda.is_available() or capi.device_count() < 1:
        raise SystemExit("time_orb_detector.py needs a GPU: dsopp_amd has no CPU fallback")
    torch.cuda.init()
    stream = torch.cuda.Stream()
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        # the pyramid keeps the grey image of a frame of twice the size resized at ratio 0.5: the image a bootstrap frame detects on
        tr = capi.Transformer((2 * W, 2 * H), resize_ratio=0.5, crop_levels=0, stream=stream.cuda_stream)
        pyramids = []
        for seed in range(3):
            p = capi.Pyramid(W, H, 1, stream=stream.cuda_stream)
            p.build_transformed(None, tr, texture(2 * W, 2 * H, seed, cell=32))
            pyramids.append(p)
        kept = [p.get_image(1) for p in pyramids]
        det = capi.OrbDetector(W, H, stream=stream.cuda_stream)
        dev = {"detect_from_pyramid": [], "detect": []}
        host = {"detect_from_pyramid": [], "detect": []}
        found = []
        for k in range(args.warmup + args.calls):
            for what in ("detect_from_pyramid", "detect"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                t0 = time.perf_counter()
                xy, level, response = det.detect(pyramids[k % 3] if what == "detect_from_pyramid" else kept[k % 3])
                t1 = time.perf_counter()
                e1.record(stream)
                e1.synchronize()
                if k >= args.warmup:
                    dev[what].append(e0.elapsed_time(e1))
                    host[what].append((t1 - t0) * 1e3)
            if k >= args.warmup:
                found.append([int((level == l).sum()) for l in range(det.num_levels)])
        out = {"size": size, "nfeatures": det.nfeatures, "levels": det.num_levels, "calls": args.calls}
        for what in ("detect_from_pyramid", "detect"):
            out[f"{what}_device_ms_median"] = float(np.median(dev[what]))
            out[f"{what}_device_ms_min_max"] = [float(np.min(dev[what])), float(np.max(dev[what]))]
            out[f"{what}_host_ms_median"] = float(np.median(host[what]))
        out["detections_per_level_mean"] = np.mean(np.array(found), axis=0).round(1).tolist()
        print(json.dumps(out), flush=True)
        det.close()
        for p in pyramids:
            p.close()
        tr.close()


if __name__ == "__main__":
    main()
