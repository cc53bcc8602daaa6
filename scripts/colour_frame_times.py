"""What a colour camera frame costs per frame beside a grey one.  One camera (a simple-radial map, then CameraResizer at --ratio and
ImageCropper of 4 levels), three forms of its frame, alternating so that all see the same machine, each timed by HIP events on the
pyramid's stream around the call (the second event is waited for) and by a host clock around call plus synchronise:
  build_transformed          the yardstick: dsopp_hip_pyramid_build_transformed of the frame as 8-bit grey (1 byte per pixel uploaded)
  build_colour               dsopp_hip_pyramid_build_colour of the frame as 8-bit BGR (3 bytes per pixel uploaded), grey kept
  build_colour_keep_colour   the same with keep_colour: the resize launch also stores the transformed BGR image
and every stage launch alone between device images, back to back, by HIP events: the colour remap and the colour resize + crop (grey
out, BGR out, both) beside their grey twins, and the plain conversion.  Before anything is timed the colour build is held to the NumPy
model of tests/colour_model.py, level by level.  Prints one JSON line.
    python scripts/colour_frame_times.py [--size 1280x1024 --ratio 0.75 --levels 4 --calls 300 --warmup 30 --dtype f64|f32]"""
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
    import colour_model as cm      # tests/colour_model.py
    import undistort_model as um   # tests/undistort_model.py
    if not torch.cuda.is_available() or capi.device_count() < 1:
        raise SystemExit("colour_frame_times.py needs a GPU: dsopp_amd has no CPU fallback")
    torch.cuda.init()
    W, H = (int(v) for v in args.size.split("x"))
    rng = np.random.default_rng(5)
    ys, xs = np.mgrid[0:H, 0:W]
    wave = lambda i, c: 128 + 60 * np.sin(xs / (17.0 + 3 * c) + i) * np.cos(ys / (23.0 - 2 * c)) + rng.normal(0, 8, (H, W))
    colour_frames = [np.ascontiguousarray(np.clip(np.stack([wave(i, c) for c in range(3)], axis=-1), 0, 255).astype(np.uint8)) for i in range(4)]
    grey_frames = [cm.bgr_to_grey(f) for f in colour_frames]
    maps = um.simple_radial_maps(W, H, 0.8 * W, 0.49 * W, 0.51 * H, -0.25, 0.06)
    und = capi.Undistorter((W, H), (W, H), *maps)
    tr = capi.Transformer((W, H), args.ratio, 4)
    w, h = tr.out_size
    F = capi.F64 if args.dtype == "f64" else capi.F32
    stream = torch.cuda.Stream()
    grey_pyramid, colour_pyramid, kept_pyramid, plain = (capi.Pyramid(w, h, args.levels, F, stream=stream.cuda_stream) for _ in range(4))

    # the colour build computes the pyramid of the model's grey image and keeps the model's colour image
    want_colour, want_grey = cm.frame(colour_frames[0], maps, args.ratio, 4)
    kept_pyramid.build_colour(und, tr, colour_frames[0], keep_colour=True)
    plain.build(want_grey)
    for level in range(plain.levels):
        assert np.array_equal(kept_pyramid.get_level(level), plain.get_level(level)), level
    assert np.array_equal(kept_pyramid.get_image(1), want_grey) and np.array_equal(kept_pyramid.get_image(3), want_colour)

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
        "build_transformed": lambda k: grey_pyramid.build_transformed(und, tr, grey_frames[k % 4]),
        "build_colour": lambda k: colour_pyramid.build_colour(und, tr, colour_frames[k % 4]),
        "build_colour_keep_colour": lambda k: kept_pyramid.build_colour(und, tr, colour_frames[k % 4], keep_colour=True),
    }
    events, wall = {n: [] for n in forms}, {n: [] for n in forms}
    for k in range(args.warmup + args.calls):
        for name, call in forms.items():
            e, t = timed(lambda: call(k))
            if k >= args.warmup:
                events[name].append(e)
                wall[name].append(t)

    # the stage launches alone, back to back
    d_bgr = torch.from_numpy(colour_frames[0]).cuda()
    d_grey = torch.from_numpy(grey_frames[0]).cuda()
    d_bgr_out, d_grey_out = torch.empty(3 * W * H, dtype=torch.uint8, device="cuda"), torch.empty(W * H, dtype=torch.uint8, device="cuda")
    same = capi.Transformer((W, H), 1.0, 0)
    s, bgr_in, grey_in, bgr_out, grey_out = stream.cuda_stream, d_bgr.data_ptr(), d_grey.data_ptr(), d_bgr_out.data_ptr(), d_grey_out.data_ptr()
    launches = {
        "remap_grey": lambda: und.undistort_device(grey_in, grey_out, stream=s),
        "remap_bgr_to_bgr": lambda: und.undistort_bgr_device(bgr_in, bgr_out, None, stream=s),
        "remap_bgr_to_grey": lambda: und.undistort_bgr_device(bgr_in, None, grey_out, stream=s),
        "resize_grey": lambda: tr.transform_device(grey_in, grey_out, capi.LINEAR, stream=s),
        "resize_bgr_to_grey": lambda: tr.transform_bgr_device(bgr_in, None, grey_out, stream=s),
        "resize_bgr_to_bgr": lambda: tr.transform_bgr_device(bgr_in, bgr_out, None, stream=s),
        "resize_bgr_to_both": lambda: tr.transform_bgr_device(bgr_in, bgr_out, grey_out, stream=s),
        "conversion": lambda: same.transform_bgr_device(bgr_in, None, grey_out, stream=s),
    }
    launch_us = {n: [] for n in launches}
    torch.cuda.synchronize()
    for repeat in range(4):   # alternating rounds: the spread between rounds is the noise of the figure
        for name, launch in launches.items():
            for _ in range(args.warmup):
                launch()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.calls):
                launch()
            e1.record(stream)
            e1.synchronize()
            launch_us[name].append(1e3 * e0.elapsed_time(e1) / args.calls)
    assert np.array_equal(d_grey_out.cpu().numpy().reshape(H, W), grey_frames[0])   # the conversion ran last

    result = dict(size=args.size, ratio=args.ratio, out_size="%dx%d" % (w, h), levels=plain.levels, dtype=args.dtype, calls=args.calls,
                  warmup=args.warmup, events_us={n: _stats(v) for n, v in events.items()}, wall_us={n: _stats(v) for n, v in wall.items()},
                  launch_us_back_to_back={n: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for n, v in launch_us.items()})
    for handle in (grey_pyramid, colour_pyramid, kept_pyramid, plain, same, tr, und):
        handle.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
