"""What resizing and cropping on the device costs per frame.  Three forms of one camera frame (a TUM-FOV map, then CameraResizer at
--ratio and ImageCropper of 4 levels), alternating so that all see the same machine, each timed by HIP events on the pyramid's stream
around the call (the second event is waited for) and by a host clock around call plus synchronise:
  build_undistorted   the chain without the new launch: dsopp_hip_pyramid_build_undistorted into a pyramid of the full size
  build_transformed   dsopp_hip_pyramid_build_transformed into a pyramid of the transformed size
  host round trip     what a caller had to do without it: dsopp_hip_undistorter_undistort (upload, remap, read-back), a resize on the
                      host, dsopp_hip_pyramid_build of the resized copy.  The host resize itself is NOT timed (the library has no host
                      statement of it outside the tests' NumPy model, which is no fair opponent): the figure is a lower bound.
and the transformer's launch alone (dsopp_hip_transformer_transform_device between two device images) by HIP events, back to back.
Prints one JSON line.
    python scripts/time_transform.py [--size 1280x1024 --ratio 0.75 --levels 4 --calls 300 --warmup 30 --dtype f64|f32]"""
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


def _stats(seconds):
    us = 1e6 * np.asarray(seconds)
    return dict(median=float(np.median(us)), p10=float(np.percentile(us, 10)), p90=float(np.percentile(us, 90)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1280x1024")
    ap.add_argument("--ratio", type=float, default=0.75)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--dtype", choices=("f64", "f32"), default="f64")
    args = ap.parse_args()
    import torch  # plumbing: streams, device buffers and events; its HIP runtime comes up before the library's
    from dsopp_amd import capi
    import transform_model as tm   # tests/transform_model.py
    import undistort_model as um   # tests/undistort_model.py
    if not torch.cuda.is_available() or capi.device_count() < 1:
        raise SystemExit("time_transform.py needs a GPU: dsopp_amd has no CPU fallback")
    torch.cuda.init()
    W, H = (int(v) for v in args.size.split("x"))
    rng = np.random.default_rng(5)
    ys, xs = np.mgrid[0:H, 0:W]
    frames = [np.clip(128 + 60 * np.sin(xs / 17.0 + i) * np.cos(ys / 23.0) + rng.normal(0, 8, (H, W)), 0, 255).astype(np.uint8) for i in range(4)]
    map_x, map_y = um.tum_fov_maps(W, H, 0.7 * W, 0.72 * H, 0.51 * W, 0.48 * H, 0.93)
    und = capi.Undistorter((W, H), (W, H), map_x, map_y)
    tr = capi.Transformer((W, H), args.ratio, 4)
    w, h = tr.out_size
    F = capi.F64 if args.dtype == "f64" else capi.F32
    stream = torch.cuda.Stream()
    full = capi.Pyramid(W, H, args.levels, F, stream=stream.cuda_stream)
    transformed = capi.Pyramid(w, h, args.levels, F, stream=stream.cuda_stream)
    small = capi.Pyramid(w, h, args.levels, F, stream=stream.cuda_stream)

    # the transformed build computes the pyramid of the model's image
    resized = [tm.transform_image(um.remap(f, map_x, map_y), args.ratio, 4) for f in frames]
    assert np.array_equal(tr.transform_image(und.undistort(frames[0])), resized[0])
    transformed.build_transformed(und, tr, frames[0])
    small.build(resized[0])
    for level in range(small.levels):
        assert np.array_equal(transformed.get_level(level), small.get_level(level)), level

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        torch.cuda.synchronize()
        return 1e-3 * e0.elapsed_time(e1), time.perf_counter() - t0

    forms = {
        "build_undistorted": lambda k: full.build_undistorted(und, frames[k % 4]),
        "build_transformed": lambda k: transformed.build_transformed(und, tr, frames[k % 4]),
        "host_round_trip_without_the_resize": lambda k: (und.undistort(frames[k % 4]), small.build(resized[k % 4])),
    }
    events, wall = {n: [] for n in forms}, {n: [] for n in forms}
    for k in range(args.warmup + args.calls):
        for name, call in forms.items():
            e, t = timed(lambda: call(k))
            if k >= args.warmup:
                events[name].append(e)
                wall[name].append(t)

    d_in = torch.from_numpy(und.undistort(frames[0])).cuda()
    d_out = torch.empty(w * h, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for _ in range(args.warmup):
        tr.transform_device(d_in.data_ptr(), d_out.data_ptr(), capi.LINEAR, stream=stream.cuda_stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(args.calls):
        tr.transform_device(d_in.data_ptr(), d_out.data_ptr(), capi.LINEAR, stream=stream.cuda_stream)
    e1.record(stream)
    e1.synchronize()
    assert np.array_equal(d_out.cpu().numpy().reshape(h, w), resized[0])

    result = dict(size=args.size, ratio=args.ratio, out_size="%dx%d" % (w, h), levels=small.levels, dtype=args.dtype, calls=args.calls,
                  warmup=args.warmup, events_us={n: _stats(v) for n, v in events.items()}, wall_us={n: _stats(v) for n, v in wall.items()},
                  transform_launch_us_back_to_back=1e3 * e0.elapsed_time(e1) / args.calls,
                  host_resize="not timed: no host statement of the arithmetic exists outside the tests' NumPy model")
    for handle in (full, transformed, small, tr, und):
        handle.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
