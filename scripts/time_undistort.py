"""What undistorting on the device costs per frame: wall time of Pyramid.build and of Pyramid.build_undistorted (the same frame through
dsopp_hip_pyramid_build_undistorted: a pinned copy and upload of the distorted image, the remap launch, the same level kernels), each a
host clock around the call plus a device synchronise, alternating between the two so that both see the same machine; and the remap
launch alone (dsopp_hip_undistorter_undistort_device between two device images) by HIP events on one stream, one launch per event
pair and --calls launches back to back.  The remap moves 8 bytes of table, at most 4 bytes of source lines and 1 byte of output per
pixel; its share of the HBM peak is printed for the table + one read + one write of the image (10 bytes per pixel).
No host remap is timed: the library has no host statement of the arithmetic outside the tests' NumPy model, which is no fair opponent.
Prints one JSON line.
    python scripts/time_undistort.py [--size 1280x1024 --levels 4 --calls 300 --warmup 30 --dtype f64|f32]"""
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

HBM_PEAK_BYTES_PER_S = 8.0e12


def _stats(seconds):
    us = 1e6 * np.asarray(seconds)
    return dict(median=float(np.median(us)), p10=float(np.percentile(us, 10)), p90=float(np.percentile(us, 90)), mean=float(us.mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1280x1024")
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--dtype", choices=("f64", "f32"), default="f64")
    args = ap.parse_args()
    import torch  # plumbing: device buffers and events; its HIP runtime comes up before the library's
    from dsopp_amd import capi
    import undistort_model as um   # the camera map (tests/undistort_model.py)
    if not torch.cuda.is_available() or capi.device_count() < 1:
        raise SystemExit("time_undistort.py needs a GPU: dsopp_amd has no CPU fallback")
    torch.cuda.init()
    W, H = (int(v) for v in args.size.split("x"))
    rng = np.random.default_rng(5)
    # a smooth image with texture, and the TUM-FOV map of a wide-angle camera of this size
    ys, xs = np.mgrid[0:H, 0:W]
    frames = [np.clip(128 + 60 * np.sin(xs / 17.0 + i) * np.cos(ys / 23.0) + rng.normal(0, 8, (H, W)), 0, 255).astype(np.uint8) for i in range(4)]
    map_x, map_y = um.tum_fov_maps(W, H, 0.7 * W, 0.72 * H, 0.51 * W, 0.48 * H, 0.93)
    und = capi.Undistorter((W, H), (W, H), map_x, map_y)
    F = capi.F64 if args.dtype == "f64" else capi.F32
    plain, undistorted = capi.Pyramid(W, H, args.levels, F), capi.Pyramid(W, H, args.levels, F)

    # the two builds compute the same pyramid when the plain one is handed the remapped frame
    remapped = und.undistort(frames[0])
    assert np.array_equal(remapped, um.remap(frames[0], map_x, map_y))
    plain.build(remapped)
    undistorted.build_undistorted(und, frames[0])
    for level in range(plain.levels):
        assert np.array_equal(plain.get_level(level), undistorted.get_level(level)), level

    t_plain, t_und = [], []
    for k in range(args.warmup + args.calls):
        img = frames[k % len(frames)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plain.build(img)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        undistorted.build_undistorted(und, img)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if k >= args.warmup:
            t_plain.append(t1 - t0)
            t_und.append(t2 - t1)

    # the remap launch alone
    stream = torch.cuda.Stream()
    d_in = torch.from_numpy(frames[0]).cuda()
    d_out = torch.empty(W * H, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    single = []
    with torch.cuda.stream(stream):
        for k in range(args.warmup + args.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            und.undistort_device(d_in.data_ptr(), d_out.data_ptr(), stream=stream.cuda_stream)
            e1.record(stream)
            e1.synchronize()
            if k >= args.warmup:
                single.append(1e-3 * e0.elapsed_time(e1))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.calls):
            und.undistort_device(d_in.data_ptr(), d_out.data_ptr(), stream=stream.cuda_stream)
        e1.record(stream)
        e1.synchronize()
        back_to_back_us = 1e3 * e0.elapsed_time(e1) / args.calls
    assert np.array_equal(d_out.cpu().numpy().reshape(H, W), remapped)

    remap_bytes = 10 * W * H
    least_us = 1e6 * remap_bytes / HBM_PEAK_BYTES_PER_S
    result = dict(size=args.size, levels=plain.levels, dtype=args.dtype, calls=args.calls, warmup=args.warmup,
                  build_us=_stats(t_plain), build_undistorted_us=_stats(t_und),
                  undistorted_minus_plain_us_median=float(np.median(1e6 * (np.asarray(t_und) - np.asarray(t_plain)))),
                  remap_launch_us_events=_stats(single), remap_launch_us_back_to_back=back_to_back_us,
                  remap_bytes=remap_bytes, remap_least_us_at_8TBps=least_us,
                  remap_share_of_hbm_peak_back_to_back=least_us / back_to_back_us,
                  remap_share_of_hbm_peak_single=least_us / float(np.median(single) * 1e6),
                  host_remap="not timed: no host statement of the arithmetic exists outside the tests' NumPy model")
    und.close()
    plain.close()
    undistorted.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
