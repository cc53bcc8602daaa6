"""What building an undistorter costs, once per camera: dsopp_hip_undistorter_create_from_model (the maps evaluated and folded on the
device: one launch, nothing uploaded but the kernel's arguments) without and with the two float maps read back, beside the path it
replaces: the maps built on the host — here by the NumPy code of tests/camera_remap_model.py, which stands for the reference's host loop
only in what it computes, not in its speed — then folded by dsopp_hip_undistorter_create in a host loop and uploaded, 8 bytes per pixel.
Each figure is the median of --calls blocking calls under a host clock (every call ends in the library's own stream synchronise), the
variants alternating; the launch is also bracketed by two HIP events on the caller's stream, an interval that holds the kernel and the
host's allocation of the table between the two records.  TUM-FOV camera; the first call of each variant is warm-up.
Prints one JSON line per size.
    python scripts/time_camera_remap.py [--sizes 640x480,1280x1024 --calls 20 --commit ID]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)


def _median_us(seconds):
    return float(np.median(1e6 * np.asarray(seconds)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="640x480,1280x1024")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--commit", default=None, help="the commit the figures belong to (default: git's HEAD, where the tree is a checkout)")
    args = ap.parse_args()
    import torch  # plumbing: the caller's stream and its events; its HIP runtime comes up before the library's
    from dsopp_amd import capi
    import camera_remap_model as cm
    if not torch.cuda.is_available() or capi.device_count() < 1:
        raise SystemExit("time_camera_remap.py needs a GPU: dsopp_amd has no CPU fallback")
    torch.cuda.init()
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
        except OSError:
            pass
    stream = torch.cuda.Stream()
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        camera = cm.CAMERAS["fov"](W, H)
        model = capi.CameraModel.tum_fov((W, H), *camera[1:])
        t_device, t_device_maps, t_host_model, t_host_create, t_events = [], [], [], [], []
        for k in range(args.calls + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a = capi.Undistorter.from_model(model)
            t1 = time.perf_counter()
            b = capi.Undistorter.from_model(model, maps=True)
            t2 = time.perf_counter()
            tab = cm.Tables(W, H, camera)
            t3 = time.perf_counter()
            c = capi.Undistorter((W, H), (W, H), tab.map_x, tab.map_y)
            t4 = time.perf_counter()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            d = capi.Undistorter.from_model(model, stream=stream.cuda_stream)
            e1.record(stream)
            e1.synchronize()
            if k == 0:   # the three tables agree wherever the device's atan2 and NumPy's give one float (everywhere, at the tested sizes)
                image = np.random.default_rng(3).integers(0, 256, (H, W)).astype(np.uint8)
                out = a.undistort(image)
                assert np.array_equal(out, b.undistort(image)) and np.array_equal(out, d.undistort(image))
                agree = float((out == c.undistort(image)).mean())
            else:
                t_device.append(t1 - t0)
                t_device_maps.append(t2 - t1)
                t_host_model.append(t3 - t2)
                t_host_create.append(t4 - t3)
                t_events.append(1e-3 * e0.elapsed_time(e1))
            for u in (a, b, c, d):
                u.close()
        print(json.dumps(dict(
            size=size, camera="tum_fov", calls=args.calls, date=time.strftime("%Y-%m-%d"), commit=commit,
            create_from_model_us=_median_us(t_device), create_from_model_with_maps_us=_median_us(t_device_maps),
            events_round_create_from_model_us=_median_us(t_events),
            replaced_path_us=dict(numpy_maps=_median_us(t_host_model), undistorter_create=_median_us(t_host_create),
                                  total=_median_us(np.asarray(t_host_model) + np.asarray(t_host_create))),
            bytes_uploaded=dict(create_from_model=0, undistorter_create=8 * W * H),
            share_of_remapped_bytes_equal_to_the_host_maps_table=agree)), flush=True)


if __name__ == "__main__":
    main()
