"""What the tracker's debug views cost on the device, against the copy the host route cannot avoid.  At --size (1280x1024) a 7-keyframe,
~2000-point window is bundle-adjusted and its reference depth maps are created on the device, as bench.py --full builds them for the
tracker; the keyframe's pyramid keeps its 8-bit grey image.  In one process, after a warm-up, alternating so that all see the same machine,
each timed by a host clock around a call that ends in a synchronise:
  keyframe_view    (a) DebugViews.keyframe, host-out: two launches and the read-back of the 3 W H byte image
  get_level0       (b) DepthMaps.get_level(0): the two f64 planes to the host, 16 W H bytes — unchanged code, what debugCurrentKeyframe on the
                   host has to wait for before it draws a single circle (the reference's drawing and colour map come on top; they need OpenCV
                   and are NOT timed)
  frame_view       DebugViews.frame, host-out: one launch and the same read-back
  get_image        Pyramid.get_image(1): the W H byte grey image to the host, what debugCurrentFrame on the host starts from
and the three launches alone, back to back by HIP events between device buffers.  Prints one JSON line; (a) counts as below (b) when the
medians differ by more than the larger of the two p10 .. p90 spreads.  For the kernel times run it under
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/time_debug_views.py --calls 30
    python scripts/time_debug_views.py [--size 1280x1024 --calls 100 --warmup 10]"""
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
    return dict(median=float(np.median(us)), p10=float(np.percentile(us, 10)), p90=float(np.percentile(us, 90)), min=float(us.min()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1280x1024")
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-check", action="store_true", help="skip the comparison with the NumPy model (tests/debug_views_model.py)")
    args = ap.parse_args()
    assert args.calls >= 30, "at least 30 repetitions of each form"
    import torch  # plumbing: streams, device buffers and events; its HIP runtime comes up before the library's
    from dsopp_amd import capi, synthetic as syn
    import debug_views_model as dv   # tests/debug_views_model.py
    if not torch.cuda.is_available() or capi.device_count() < 1:
        raise SystemExit("time_debug_views.py needs a GPU: dsopp_amd has no CPU fallback")
    torch.cuda.init()
    W, H = (int(v) for v in args.size.split("x"))
    L = 5
    win = syn.make_window(num_frames=8, num_points=2288, width=W, height=H, seed=3)
    win.frames.pop()                                   # (bench.py's tracker timing: the eighth frame is the one it tracks)
    g = capi.HipWindow(capi.default_pba_options())
    syn.load_window(g, win)
    g.solve()
    maps = g.create_reference_depth_maps(L)
    grey = np.ascontiguousarray(win.frames[-1].image_u8)
    pyr = capi.Pyramid(W, H, L)
    und = capi.Undistorter((W, H), (W, H))
    pyr.build_undistorted(und, grey)
    rng = np.random.default_rng(1)
    mask = (rng.random((H, W)) < 0.9).astype(np.uint8)
    pyr.set_mask(0, mask)
    views = capi.DebugViews(W, H)

    ids, wgt = maps.get_level(0)
    cells = int((ids > 0).sum())
    img, M, got_cells = views.keyframe(pyr, maps)
    assert got_cells == cells
    if not args.no_check:
        want, wM, _ = dv.keyframe_view(grey, ids, wgt, 0.0)
        assert img.tobytes() == want.tobytes() and M == wM, "the keyframe view differs from the model"
        assert views.frame(pyr).tobytes() == dv.frame_view(grey, mask).tobytes(), "the frame view differs from the model"

    def timed(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()                                          # (every form ends in a synchronise of its own stream)
        return time.perf_counter() - t0

    forms = {
        "keyframe_view": lambda: views.keyframe(pyr, maps),
        "get_level0": lambda: maps.get_level(0),
        "frame_view": lambda: views.frame(pyr),
        "get_image": lambda: pyr.get_image(1),
    }
    wall = {n: [] for n in forms}
    for k in range(args.warmup + args.calls):
        for name, call in forms.items():
            t = timed(call)
            if k >= args.warmup:
                wall[name].append(t)

    # the launches alone: device in, device out, back to back on one stream
    stream = torch.cuda.Stream()
    d_grey = torch.from_numpy(grey.reshape(-1).copy()).cuda()
    d_mask = torch.from_numpy(mask.reshape(-1).copy()).cuda()
    d_out = torch.empty(3 * W * H, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    launches = {}
    for name, call in {"keyframe_view_two_launches": lambda: views.keyframe_device(d_grey.data_ptr(), maps, d_out.data_ptr(), stream.cuda_stream),
                       "frame_view_launch": lambda: views.frame_device(d_grey.data_ptr(), d_mask.data_ptr(), d_out.data_ptr(), stream.cuda_stream)}.items():
        for _ in range(args.warmup):
            call()
        stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.calls):
            call()
        e1.record(stream)
        e1.synchronize()
        launches[name] = 1e3 * e0.elapsed_time(e1) / args.calls

    stats = {n: _stats(v) for n, v in wall.items()}
    a, b = stats["keyframe_view"], stats["get_level0"]
    spread = max(a["p90"] - a["p10"], b["p90"] - b["p10"])
    result = dict(size=args.size, calls=args.calls, warmup=args.warmup, map_cells=cells, maximum_idepth=views.maximum_idepth,
                  bytes=dict(keyframe_view_read_back=3 * W * H, get_level0=16 * W * H, get_image=W * H),
                  wall_us=stats, launches_us_back_to_back=launches,
                  keyframe_view_over_get_level0=a["median"] / b["median"], spread_us=spread,
                  keyframe_view_below_get_level0_by_more_than_the_spread=bool(b["median"] - a["median"] > spread),
                  host_drawing="not timed: the reference's cv::circle loop and cv::applyColorMap need OpenCV; they come on top of get_level0")
    for handle in (views, pyr, und, maps, g):
        handle.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
