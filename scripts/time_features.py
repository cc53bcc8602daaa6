"""Wall time of the keyframe-candidate selection on the device, per call: dsopp_hip_feature_extractor_extract (upload, Sobel, window
first hits, compaction, count and list read-back, host shuffle) and dsopp_hip_immature_set_create_from_features (set allocation, ROI
scan, build from pyramid level 0), with the reference's default configuration (density 1500, quantile 0.6).  Each is the median of
--calls calls after --warmup, on frames of a rendered scene; the extractor alternates between frames so that every call adapts.
--kind eigen times the eigen extractor (dsopp_hip_feature_extractor_create_eigen: its own pyramid, threshold map, the window walk
and up to two passes) instead, and reports its pass statistics.  Prints one JSON line per size.
    python scripts/time_features.py [--kind sobel|eigen --sizes 640x480,1280x1024 --calls 200 --warmup 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=("sobel", "eigen"), default="sobel")
    ap.add_argument("--sizes", default="640x480,1280x1024")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--density", type=float, default=1500.0)
    ap.add_argument("--quantile", type=float, default=0.6)
    args = ap.parse_args()
    import torch  # the frames are rendered with torch (plumbing); its HIP runtime comes up before the library's
    from dsopp_amd import capi, synthetic as syn
    if not torch.cuda.is_available() or capi.device_count() < 1:
        raise SystemExit("time_features.py needs a GPU: dsopp_amd has no CPU fallback")
    torch.cuda.init()
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        scene = syn.Scene.make(W, H, seed=11)
        frames = []
        for i in range(4):
            T = syn.se3_exp(np.array([0.03 * i, -0.01 * i, 0.02 * i, 0.002 * i, -0.003 * i, 0.001 * i]))
            img, _ = scene.render_torch(T, 0.0, 0.0, "cuda")
            frames.append(np.clip(np.round(img), 0, 255).astype(np.uint8))
        if args.kind == "eigen":
            ex = capi.EigenFeatureExtractor(W, H, args.density)
        else:
            ex = capi.FeatureExtractor(W, H, args.density, args.quantile)
        pyr = capi.Pyramid(W, H, 1)
        pyr.build(frames[0])
        ex.extract(frames[0])
        t_extract, t_build, n_features, n_landmarks = [], [], [], []
        for k in range(args.warmup + args.calls):
            img = frames[k % len(frames)]
            t0 = time.perf_counter()
            xy = ex.extract(img)
            t1 = time.perf_counter()
            s = capi.ImmatureSet.from_features(ex, pyr, scene.intrinsics)
            t2 = time.perf_counter()
            s.close()
            if k >= args.warmup:
                t_extract.append(t1 - t0)
                t_build.append(t2 - t1)
                n_features.append(len(xy))
                n_landmarks.append(s.n)
        st = ex.state()
        if args.kind == "eigen":
            extra = dict(eigen_stats_last=ex.stats())
        else:
            extra = dict(quantile=args.quantile, grad_norm_threshold=st["grad_norm_threshold"])
        ex.close()
        pyr.close()
        print(json.dumps(dict(kind=args.kind, size=size, calls=args.calls, density=args.density,
                              extract_us_median=1e6 * float(np.median(t_extract)), extract_us_p10=1e6 * float(np.percentile(t_extract, 10)),
                              extract_us_p90=1e6 * float(np.percentile(t_extract, 90)),
                              from_features_us_median=1e6 * float(np.median(t_build)), from_features_us_p10=1e6 * float(np.percentile(t_build, 10)),
                              from_features_us_p90=1e6 * float(np.percentile(t_build, 90)),
                              features_median=int(np.median(n_features)), landmarks_median=int(np.median(n_landmarks)),
                              window_size=st["window_size"], **extra)), flush=True)


if __name__ == "__main__":
    main()
