"""What the map costs on the device (dsopp_hip_map_*, row o-2), against what a caller of the window's getters does without it.  The
window, the map and the events share one stream; every form is timed by HIP events on that stream and by a host clock around the call
and a synchronise, read-back included, median of --calls (100):
  export_filter_off / _on   Map export of --keyframes (500) x --records (2000) records loaded by set_records: world frame, image colours,
                            all seven outputs to the host, without and with the exporter's filter (5e-8, 0.15)
  update                    Map.update of a 7-keyframe / 2000-landmark window at 640 x 480 (records exist: the steady state)
  seven_frame_updates       HipWindow.get_frame_update for each of the 7 keyframes: what a caller does today before it can apply the
                            landmark rules on the host (which are NOT timed)
both of the last two in two states of the window: right after solve(), which prefetches the getters' data behind its own synchronise
(the getters are then host copies), and after a flag refresh of one keyframe (set_landmarks), which invalidates the prefetch.
Prints one JSON line.
    python scripts/time_point_cloud.py [--keyframes 500 --records 2000 --calls 100 --warmup 10]"""
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


def _stats(values):
    v = np.asarray(values, dtype=np.float64)
    return dict(median=float(np.median(v)), p10=float(np.percentile(v, 10)), p90=float(np.percentile(v, 90)), min=float(v.min()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=500)
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    import torch  # plumbing: the stream and its events; its HIP runtime comes up before the library's
    from dsopp_amd import capi, synthetic as syn
    import point_cloud_model as pc   # tests/point_cloud_model.py
    if not torch.cuda.is_available() or capi.device_count() < 1:
        raise SystemExit("time_point_cloud.py needs a GPU: dsopp_amd has no CPU fallback")
    torch.cuda.init()
    stream = torch.cuda.Stream()

    def timed(call, prepare=None):
        """(device microseconds between two events on the stream, host microseconds until the stream is idle)"""
        dev, wall = [], []
        for k in range(args.warmup + args.calls):
            if prepare is not None:
                prepare()
            stream.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            t1 = time.perf_counter()
            if k >= args.warmup:
                dev.append(1e3 * e0.elapsed_time(e1))
                wall.append(1e6 * (t1 - t0))
        return dict(events_us=_stats(dev), wall_us=_stats(wall))

    # ---- export --------------------------------------------------------------------------------------------------------------------
    rng = np.random.default_rng(7)
    K, N = args.keyframes, args.records
    m = capi.Map(stream=stream.cuda_stream)
    first = None
    for k in range(K):
        q = rng.normal(size=4)
        pose = np.concatenate([q / np.linalg.norm(q), rng.normal(size=3) * 20])
        flags = rng.choice(np.array([0, 0, 0, 1, 1, 1, 2, 3], dtype=np.uint8), size=N)
        rec = dict(uv=rng.uniform(0, 640, (N, 2)), idepth=rng.uniform(0.02, 2.0, N), variance=np.exp(rng.uniform(np.log(1e-9), np.log(1e-6), N)),
                   relative_baseline=rng.uniform(0.0, 0.5, N), flags=flags, type=rng.integers(0, 20, N).astype(np.uint8),
                   rgb=rng.integers(0, 256, (N, 3)).astype(np.uint8))
        intr = np.array([448.0, 448.0, 320.0, 240.0])
        m.set_records(k, intr, pose, **rec)
        if first is None:
            first = pc.keyframe_from_records(k, intr, pose, **rec)
    total = K * N
    arrays = {name: np.zeros((total, w) if w > 1 else total, dtype=dt) for name, dt, w in capi.Map.OUTPUTS}
    per_kf = np.zeros(K, dtype=np.int32)
    export = {}
    for name, on in (("export_filter_off", 0), ("export_filter_on", 1)):
        o = m.export_options(classes=pc.CLASS_ACTIVE | pc.CLASS_MARGINALIZED, apply_filters=on, frame=pc.FRAME_WORLD, colours=pc.COLOURS_IMAGE)
        counts = []

        def call():
            rc, n = m.export_raw(o, None, total, arrays, per_keyframe_counts=per_kf)
            assert rc == 0
            counts.append(n)
        export[name] = timed(call)
        export[name]["points"] = int(counts[-1])
        export[name]["read_back_bytes"] = int(counts[-1]) * (24 + 3 + 1 + 8 + 8 + 4 + 4)
        want = pc.export([first], apply_filters=bool(on), colours=pc.COLOURS_IMAGE)   # the first keyframe against the model
        n0 = want["count"]
        assert per_kf[0] == n0 and all(arrays[k][:n0].tobytes() == want[k].tobytes() for k in arrays), "the export differs from the model"
    m.close()

    # ---- update against seven read-backs -------------------------------------------------------------------------------------------
    win = syn.make_window(num_frames=7, num_points=2000, width=640, height=480, seed=3)
    w = capi.HipWindow(capi.default_pba_options(), stream=stream.cuda_stream)
    syn.load_window(w, win)
    ids = w.frame_ids()
    m = capi.Map(stream=stream.cuda_stream)
    for fid in ids:
        m.add_keyframe(w, fid)
    w.solve()
    m.update(w)
    targets = {fid: [t for t in ids if t != fid] for fid in ids}
    f0 = win.frames[0]
    zeros = np.zeros(len(f0.uv), dtype=np.uint8)

    def refresh():
        w.solve()
        w.set_landmarks(f0.frame_id, f0.uv, f0.idepth_init, f0.patch, zeros)

    window = {}
    for state, prepare in (("after_solve", w.solve), ("after_flag_refresh", refresh)):
        window[state] = dict(update=timed(lambda: m.update(w), prepare),
                             seven_frame_updates=timed(lambda: [w.get_frame_update(fid, targets[fid]) for fid in ids], prepare))
        a, b = window[state]["update"]["wall_us"], window[state]["seven_frame_updates"]["wall_us"]
        window[state]["update_over_seven_frame_updates"] = a["median"] / b["median"]
    landmarks = {int(fid): w.num_landmarks(fid) for fid in ids}
    m.close()
    w.close()
    print(json.dumps(dict(keyframes=K, records_per_keyframe=N, calls=args.calls, warmup=args.warmup, export=export, window_landmarks=landmarks,
                          window=window, host_rules="not timed: the landmark rules a caller of get_frame_update applies on the host come on top")),
          flush=True)


if __name__ == "__main__":
    main()
