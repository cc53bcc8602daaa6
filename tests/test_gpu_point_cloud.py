"""The map on the device (point_cloud.hip, dsopp_hip_map_*) against the NumPy statement of tests/point_cloud_model.py: counts, indices,
flags, types and colours exactly, positions, baselines and variances as bit patterns — the arithmetic is stated operation by operation,
so there is no tolerance.  The export is reached through set_records (sizes at wavefront and chunk edges, more chunks than the scanning
workgroup has threads), the update through real windows fed to the model by the window's own getters."""
import ctypes as C
import functools

import numpy as np
import pytest

import marginalization_model as mm
import point_cloud_model as pc
from dsopp_amd import synthetic as syn

pytestmark = pytest.mark.gpu

ERR_INVALID_ARGUMENT, ERR_NOT_FOUND, ERR_CAPACITY, ERR_STATE = -1, -2, -5, -6
CHUNK = 256
OUTPUTS = ("xyz", "rgb", "type", "relative_baseline", "idepth_variance", "keyframe_index", "record_index")


def _same(a, b):
    """equal as bit patterns (NaN and -0.0 included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def random_keyframe(seed, fid, n, rgb=True, plain=False):
    """records at every edge of the predicate: idepth 0, below 1e-16 and negative, variance and baseline at the filters' thresholds"""
    rng = np.random.default_rng(1000 * seed + fid)
    q = rng.normal(size=4)
    pose = np.concatenate([q / np.linalg.norm(q), rng.normal(size=3) * 5])
    intr = np.array([rng.uniform(40, 50), rng.uniform(40, 50), 32 + rng.normal(), 24 + rng.normal()])
    uv = rng.uniform(0, 64, size=(n, 2))
    idepth = rng.uniform(0.05, 2.0, size=n)
    variance = np.exp(rng.uniform(np.log(1e-9), np.log(1e-6), size=n))
    baseline = rng.uniform(0.0, 0.4, size=n)
    flags = rng.choice(np.array([0, 0, 0, 1, 1, 2, 3], dtype=np.uint8), size=n)
    if not plain:
        pick = lambda share: rng.random(n) < share  # noqa: E731
        idepth[pick(0.05)] = 0.0
        idepth[pick(0.03)] = 5e-17
        idepth[pick(0.03)] = -0.3
        variance[pick(0.05)] = 5e-8
        baseline[pick(0.05)] = 0.1
        baseline[pick(0.05)] = 0.15
    return pc.keyframe_from_records(fid, intr, pose, uv, idepth, variance, baseline, flags, rng.integers(0, 256, n).astype(np.uint8),
                                    rng.integers(0, 256, (n, 3)).astype(np.uint8) if rgb else None)


def load(capi, keyframes, **map_options):
    m = capi.Map(**map_options)
    for kf in keyframes:
        m.set_records(kf.frame_id, kf.intrinsics, kf.pose, kf.uv, kf.idepth, kf.variance, kf.relative_baseline, kf.flags, kf.type,
                      kf.rgb if kf.has_image else None)
    return m


def check_export(m, keyframes, ids=None, min_relative_baseline=0.1, **options):
    """the host form against the model over `keyframes` (the exported ones, in order): every output, count and per-keyframe counts"""
    want = pc.export(keyframes, min_relative_baseline=min_relative_baseline, **options)
    got = m.export(ids, **options)
    assert got["count"] == want["count"], (got["count"], want["count"])
    assert got["per_keyframe_counts"].tolist() == want["per_keyframe_counts"].tolist()
    for name in OUTPUTS:
        assert _same(got[name], want[name]), name
    return want


@functools.lru_cache(maxsize=None)
def big_keyframes():
    return tuple(random_keyframe(9, fid, n) for fid, n in ((0, 40000), (1, 0), (2, 26100)))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1])
def test_export_at_wave_and_chunk_edges(n):
    from dsopp_amd import capi
    kfs = [random_keyframe(1, 5, n)]
    m = load(capi, kfs)
    assert m.keyframe_ids() == [5] and m.num_records(5) == n
    want = check_export(m, kfs, classes=pc.CLASS_ALL)
    check_export(m, kfs, classes=pc.CLASS_ALL, frame=pc.FRAME_KEYFRAME, colours=pc.COLOURS_IMAGE)
    if n >= 63:
        assert 0 < want["count"] < n
    rec = m.records(5)
    for name in ("uv", "idepth", "variance", "relative_baseline", "flags", "type", "rgb"):
        assert _same(rec[name], getattr(kfs[0], name)), name
    assert _same(rec["pose"], kfs[0].pose) and _same(rec["intrinsics"], kfs[0].intrinsics) and rec["has_image"] and rec["finalised"]
    m.close()


def test_more_chunks_than_the_scanning_workgroup_has_threads():
    """66 100 records in 259 chunks: the last workgroup's scan takes two rounds"""
    from dsopp_amd import capi
    kfs = list(big_keyframes())
    assert sum((k.n + CHUNK - 1) // CHUNK for k in kfs) > CHUNK
    m = load(capi, kfs)
    want = check_export(m, kfs, classes=pc.CLASS_ALL, colours=pc.COLOURS_IMAGE)
    assert want["count"] > 30000 and want["per_keyframe_counts"][1] == 0
    m.close()


def test_empty_keyframes_filters_masks_colours_frames_and_id_lists():
    from dsopp_amd import capi
    sizes = [0, 70, 0, 300, 0, 257, 0]
    kfs = [random_keyframe(2, 10 + i, n) for i, n in enumerate(sizes)]
    m = load(capi, kfs)
    assert m.num_keyframes == len(sizes) and m.keyframe_ids() == [10 + i for i in range(len(sizes))]
    for classes in (0, 1, 2, 4, 3, 5, 6, 7):
        want = check_export(m, kfs, classes=classes)
        assert (want["count"] > 0) == (classes != 0)
    for colours in (pc.COLOURS_LANDMARK_TYPE, pc.COLOURS_CONSTANT, pc.COLOURS_SEMANTIC, pc.COLOURS_IMAGE):
        for frame in (pc.FRAME_KEYFRAME, pc.FRAME_WORLD):
            check_export(m, kfs, classes=pc.CLASS_ALL, colours=colours, frame=frame)
    # the exporter's filter on; everything filtered; a filter that passes everything
    on = check_export(m, kfs, classes=pc.CLASS_ALL, apply_filters=1)
    off = check_export(m, kfs, classes=pc.CLASS_ALL)
    assert 0 < on["count"] < off["count"]
    assert check_export(m, kfs, classes=pc.CLASS_ALL, apply_filters=1, max_idepth_variance=0.0)["count"] == 0
    assert check_export(m, kfs, classes=pc.CLASS_ALL, apply_filters=1, max_idepth_variance=1.0, min_relative_baseline_filter=-1.0)["count"] == off["count"]
    # an id list in another order than the insertion's, empty keyframes at both ends, one keyframe twice
    order = [16, 13, 10, 11, 15, 13, 12]
    by_id = {k.frame_id: k for k in kfs}
    want = check_export(m, [by_id[i] for i in order], ids=order, classes=pc.CLASS_ALL, colours=pc.COLOURS_SEMANTIC)
    assert want["per_keyframe_counts"][1] == want["per_keyframe_counts"][5] > 0
    # the map's own minimal baseline
    m2 = load(capi, kfs, min_relative_baseline=0.2)
    assert check_export(m2, kfs, min_relative_baseline=0.2, classes=pc.CLASS_ALL)["count"] < off["count"]
    # set_pose moves a keyframe's points; set_records replaces a keyframe
    kfs[3].pose = random_keyframe(3, 99, 0).pose
    m.set_pose(13, kfs[3].pose)
    kfs[1] = random_keyframe(4, 11, 129, rgb=False)
    m.set_records(11, kfs[1].intrinsics, kfs[1].pose, kfs[1].uv, kfs[1].idepth, kfs[1].variance, kfs[1].relative_baseline, kfs[1].flags, kfs[1].type)
    check_export(m, kfs, classes=pc.CLASS_ALL)
    assert not m.records(11)["has_image"]
    with pytest.raises(capi.HipError, match=f"error {ERR_STATE}"):
        m.export(colours=pc.COLOURS_IMAGE)
    check_export(m, [kfs[3], kfs[5]], ids=[13, 15], colours=pc.COLOURS_IMAGE)   # the keyframes listed have colours
    m.close()
    m2.close()


def test_nothing_filtered():
    from dsopp_amd import capi
    kfs = [random_keyframe(5, i, n, plain=True) for i, n in enumerate((CHUNK, 100))]
    for k in kfs:
        k.relative_baseline[:] = np.maximum(k.relative_baseline, 0.11)
    m = load(capi, kfs)
    assert check_export(m, kfs, classes=pc.CLASS_ALL)["count"] == CHUNK + 100
    m.close()


def _guarded(capacity):
    """every output with 8 guard entries in front and behind"""
    dt = dict(xyz=(np.float64, 3), rgb=(np.uint8, 3), type=(np.uint8, 1), relative_baseline=(np.float64, 1), idepth_variance=(np.float64, 1),
              keyframe_index=(np.int32, 1), record_index=(np.int32, 1))
    full = {k: np.frombuffer(bytes([0xA5]) * ((capacity + 16) * w * np.dtype(t).itemsize), dtype=t).copy() for k, (t, w) in dt.items()}
    inner = {k: full[k][8 * dt[k][1]:] for k in full}
    return dt, full, inner


@pytest.mark.parametrize("short", [0, 1])
def test_capacity_exact_and_one_short(short):
    from dsopp_amd import capi
    kfs = [random_keyframe(6, i, n) for i, n in enumerate((300, 0, 90))]
    m = load(capi, kfs)
    want = pc.export(kfs, classes=pc.CLASS_ALL)
    capacity = want["count"] - short
    dt, full, inner = _guarded(capacity)
    per_kf = np.zeros(3, dtype=np.int32)
    rc, count = m.export_raw(m.export_options(classes=pc.CLASS_ALL), None, capacity, inner, per_keyframe_counts=per_kf)
    assert rc == (ERR_CAPACITY if short else 0) and count == want["count"] and per_kf.tolist() == want["per_keyframe_counts"].tolist()
    for name, (t, w) in dt.items():
        a = full[name]
        guard = np.frombuffer(bytes([0xA5]) * (8 * w * np.dtype(t).itemsize), dtype=t)
        assert _same(a[:8 * w], guard) and _same(a[(8 + capacity) * w:], guard), name
        assert _same(a[8 * w:(8 + capacity) * w], want[name].reshape(-1)[:capacity * w]), name
    m.close()


def test_null_outputs():
    from dsopp_amd import capi
    kfs = [random_keyframe(7, i, n) for i, n in enumerate((257, 64))]
    m = load(capi, kfs)
    want = pc.export(kfs)
    for wanted in (("rgb",), ("xyz",), ("type", "record_index"), ()):
        got = m.export(outputs=wanted)
        assert got["count"] == want["count"] and got["per_keyframe_counts"].tolist() == want["per_keyframe_counts"].tolist()
        assert set(got) == set(wanted) | {"count", "per_keyframe_counts"}
        for name in wanted:
            assert _same(got[name], want[name]), name
    rc, count = m.export_raw(m.export_options(), None, 0, {}, count=True)   # capacity 0: the count alone
    assert rc == ERR_CAPACITY and count == want["count"]
    rc, count = m.export_raw(m.export_options(), None, 10**6, {}, count=False)
    assert rc == 0 and count is None
    m.close()


def test_device_form_repeats_and_interleaved_maps():
    import torch
    from dsopp_amd import capi
    a_kfs = [random_keyframe(8, i, n) for i, n in enumerate((300, 65, 0, 513))]
    b_kfs = [random_keyframe(9, i, n) for i, n in enumerate((1, 255))]
    a, b = load(capi, a_kfs), load(capi, b_kfs)
    opts = dict(classes=pc.CLASS_ALL, colours=pc.COLOURS_IMAGE)
    first_a, first_b = a.export(**opts), b.export(**opts)
    for _ in range(3):  # interleaved, repeated: the same bytes
        again_b, again_a = b.export(**opts), a.export(**opts)
        for name in OUTPUTS:
            assert _same(again_a[name], first_a[name]) and _same(again_b[name], first_b[name]), name
    check_export(a, a_kfs, **opts)
    check_export(b, b_kfs, **opts)
    # the device form: enqueue only, then a blocking call on the same stream
    cap = first_a["count"]
    tt = dict(xyz=torch.float64, rgb=torch.uint8, type=torch.uint8, relative_baseline=torch.float64, idepth_variance=torch.float64,
              keyframe_index=torch.int32, record_index=torch.int32)
    width = dict(xyz=3, rgb=3)
    bufs = {k: torch.zeros(cap * width.get(k, 1) + 16, dtype=t, device="cuda") for k, t in tt.items()}
    torch.cuda.synchronize()
    rc, count = a.export_raw(a.export_options(**opts), None, cap, {k: v.data_ptr() for k, v in bufs.items()}, count=False, device=True)
    assert rc == 0 and count is None
    per_kf = np.zeros(4, dtype=np.int32)
    rc, count = a.export_raw(a.export_options(**opts), None, cap, {k: v.data_ptr() for k, v in bufs.items()}, count=True, per_keyframe_counts=per_kf,
                             device=True)
    assert rc == 0 and count == cap and per_kf.tolist() == first_a["per_keyframe_counts"].tolist()
    for k, v in bufs.items():
        host = v.cpu().numpy()
        n = cap * width.get(k, 1)
        assert _same(host[:n], first_a[k].reshape(-1)), k
        assert not host[n:].any(), k
    rc, count = a.export_raw(a.export_options(**opts), None, cap - 1, {"rgb": bufs["rgb"].data_ptr()}, count=True, device=True)
    assert rc == ERR_CAPACITY and count == cap
    rc, _ = a.export_raw(a.export_options(**opts), None, cap, {"rgb": bufs["rgb"].data_ptr() + 1}, count=True, device=True)
    assert rc == ERR_INVALID_ARGUMENT
    a.close()
    b.close()


# ---- update through a real window ------------------------------------------------------------------------------------------------------

SIZES = {"64x48": (64, 48, 100, 35), "640x480": (640, 480, 2000, 300)}   # width, height, landmarks per frame, appended later


@functools.lru_cache(maxsize=None)
def _window(size):
    W, H, n, _ = SIZES[size]
    return syn.make_window(num_frames=5, num_points=5 * n, width=W, height=H, seed=21)


def _bgr(f, seed):
    rng = np.random.default_rng(seed)
    return np.clip(f.image_u8[:, :, None].astype(np.int32) + rng.integers(-20, 21, f.image_u8.shape + (3,)), 0, 255).astype(np.uint8)


def _push(w, win, f, n):
    w.push_frame(f.frame_id, f.timestamp, f.pixelinfo, None, win.scene.intrinsics, syn.mat_to_params(f.T_w_c_init), f.exposure, f.affine_init, f.fixed,
                 False)
    w.set_landmarks(f.frame_id, f.uv[:n], f.idepth_init[:n], f.patch[:n], np.zeros(n, dtype=np.uint8))


def _model_update(models, w, win, images, hists=None, weights=None, **kw):
    """the model fed with the window's own getters, frame by frame; a keyframe the window dropped is finalised"""
    held = w.frame_ids()
    for fid, kf in models.items():
        if not kf.live:
            continue
        if fid not in held:
            kf.live = False
            continue
        lm = w.get_landmarks(fid, False)
        n = len(lm["idepth"])
        pc.update_keyframe(kf, win.frames[fid].uv[:n], lm["idepth"], lm["inv_hdd"], lm["relative_baseline"], lm["flags"],
                           hist=None if hists is None else hists.get(fid), image=images.get(fid), weights=weights, **kw)
        kf.pose = w.get_pose(fid)[0]


def _check_records(m, models, only=None):
    for fid, kf in models.items():
        if only is not None and fid not in only:
            continue
        rec = m.records(fid)
        for name in ("uv", "idepth", "variance", "relative_baseline", "flags", "type", "rgb"):
            assert _same(rec[name], getattr(kf, name)), (fid, name)
        assert _same(rec["pose"], kf.pose) and _same(rec["intrinsics"], kf.intrinsics), fid
        assert rec["has_image"] == kf.has_image and rec["finalised"] == (not kf.live), fid


@pytest.mark.parametrize("size", list(SIZES))
def test_update_through_a_window(size):
    from dsopp_amd import capi
    W, H, n, extra = SIZES[size]
    win = _window(size)
    frames, spare = win.frames[:4], win.frames[4]
    w = capi.HipWindow(capi.default_pba_options())
    counts = {f.frame_id: n - (extra if f.frame_id == 1 else 0) for f in frames}
    for f in frames:
        _push(w, win, f, counts[f.frame_id])
    for r in frames:
        for t in frames:
            if r is not t:
                w.set_connection(r.frame_id, t.frame_id, np.zeros(counts[r.frame_id], dtype=np.uint8))
    # frame 0: a colour image; 1: a grey one; 2: no pyramid; 3: a pyramid that keeps no 8-bit image
    colour, grey, bare = capi.Pyramid(W, H, 1), capi.Pyramid(W, H, 1), capi.Pyramid(W, H, 1)
    colour.build_colour(None, None, _bgr(frames[0], 1), keep_colour=True)
    grey.build_colour(None, None, _bgr(frames[1], 2), keep_colour=False)
    bare.set_level(0, frames[3].pixelinfo)
    images = {0: colour.get_image(3), 1: grey.get_image(1)}
    assert images[0] is not None and images[1] is not None and grey.get_image(3) is None and bare.get_image(1) is None
    # (the synthetic motion is short: relative baselines stay below the viewer's 0.1, so this map exports from 0.01 on)
    m = capi.Map(min_relative_baseline=0.01)
    intr = win.scene.intrinsics
    models = {}
    for f, p in zip(frames, (colour, grey, None, bare)):
        m.add_keyframe(w, f.frame_id, p)
        models[f.frame_id] = pc.Keyframe(f.frame_id, intr.copy(), w.get_pose(f.frame_id)[0], has_image=f.frame_id in images)
    colour.build_colour(None, None, 255 - _bgr(frames[0], 1), keep_colour=True)   # the map copied the image: the pyramid is free again
    _check_records(m, models)   # no records yet
    assert m.export()["count"] == 0

    w.solve()
    m.update(w)
    _model_update(models, w, win, images)
    _check_records(m, models)
    print("relative baselines after the first solve:", [(float(k.relative_baseline.min()), float(k.relative_baseline.max())) for k in models.values()])
    assert all(np.any(models[i].rgb) for i in (0, 1)) and not np.any(models[2].rgb) and not np.any(models[3].rgb)
    assert all(k.n == counts[i] for i, k in models.items())

    # landmarks appended to frame 1 between two updates; the earlier records keep their uv and colour
    f1 = frames[1]
    w.set_landmarks(1, f1.uv[:n], f1.idepth_init[:n], f1.patch[:n], np.zeros(n, dtype=np.uint8))
    for t in (0, 2, 3):
        w.set_connection(1, t, np.zeros(n, dtype=np.uint8))
    w.solve()
    m.update(w)
    _model_update(models, w, win, images)
    _check_records(m, models)
    assert models[1].n == n and m.num_records(1) == n

    # the flags of choose_marginalization(apply) marginalise the records: marginalize() against the model
    got = w.choose_marginalization(capi.default_marginalization_options(strategy=mm.MAXIMUM_SIZE, minimum_size=2, maximum_size=3), apply=True)
    assert got["marginalized_ids"] == [0]
    before = {i: k.flags.copy() for i, k in models.items()}
    m.update(w)
    _model_update(models, w, win, images)
    _check_records(m, models)
    newly = models[0].flags & ~before[0] & pc.FLAG_MARGINALIZED
    assert np.all(newly == pc.FLAG_MARGINALIZED) and models[0].n == n
    # a second update changes nothing: the records are frozen
    m.update(w)
    _check_records(m, models)

    # image colours, with the export's positions in the window's current poses
    ids = m.keyframe_ids()
    assert ids == [0, 1, 2, 3]
    check_export(m, [models[0], models[1]], ids=[0, 1], min_relative_baseline=0.01, classes=pc.CLASS_ALL, colours=pc.COLOURS_IMAGE)
    with pytest.raises(capi.HipError, match=f"error {ERR_STATE}"):
        m.export([0, 2], colours=pc.COLOURS_IMAGE)
    want = check_export(m, [models[i] for i in ids], min_relative_baseline=0.01, classes=pc.CLASS_ALL)
    print("exported", want["count"], "of", sum(models[i].n for i in ids), "per keyframe", want["per_keyframe_counts"].tolist())
    assert want["count"] > 0

    # the next keyframe folds frame 0 out: finalised, its records fixed for good
    _push(w, win, spare, n)
    for f in frames[1:]:
        w.set_connection(spare.frame_id, f.frame_id, np.zeros(n, dtype=np.uint8))
        w.set_connection(f.frame_id, spare.frame_id, np.zeros(n, dtype=np.uint8))
    assert w.frame_ids() == [1, 2, 3, 4]
    m.add_keyframe(w, 4, None)
    models[4] = pc.Keyframe(4, intr.copy(), w.get_pose(4)[0])
    frozen = models[0].copy()
    w.solve()
    m.update(w)
    _model_update(models, w, win, images)
    assert not models[0].live
    _check_records(m, models)
    for name in ("idepth", "variance", "relative_baseline", "flags", "pose"):
        assert _same(getattr(models[0], name), getattr(frozen, name))
    m.update(w)
    _check_records(m, models)
    check_export(m, [models[i] for i in m.keyframe_ids()], min_relative_baseline=0.01, classes=pc.CLASS_ALL, colours=pc.COLOURS_LANDMARK_TYPE,
                 apply_filters=1, max_idepth_variance=1e-3, min_relative_baseline_filter=0.0)
    for h in (m, w, colour, grey, bare):
        h.close()


def test_update_without_uncertainty_and_with_channels():
    from dsopp_amd import capi
    win = _window("64x48")
    for kw in (dict(estimate_uncertainty=0), dict(channels=3)):
        w = capi.HipWindow(capi.default_pba_options())
        for f in win.frames[:3]:
            _push(w, win, f, 100)
        for r in win.frames[:3]:
            for t in win.frames[:3]:
                if r is not t:
                    w.set_connection(r.frame_id, t.frame_id, np.zeros(100, dtype=np.uint8))
        m = capi.Map(**kw)
        models = {}
        for f in win.frames[:3]:
            m.add_keyframe(w, f.frame_id)
            models[f.frame_id] = pc.Keyframe(f.frame_id, win.scene.intrinsics.copy(), w.get_pose(f.frame_id)[0])
        w.solve()
        m.update(w)
        _model_update(models, w, win, {}, estimate_uncertainty=bool(kw.get("estimate_uncertainty", 1)), channels=kw.get("channels", 1))
        _check_records(m, models)
        m.close()
        w.close()


def test_types_follow_the_class_observations():
    from dsopp_amd import capi
    W, H = 64, 48
    win = _window("64x48")
    frames = win.frames[:4]
    rng = np.random.default_rng(33)
    w = capi.HipWindow(capi.default_pba_options())
    s = capi.Semantics(W, H, 1, None, None)
    keep = [s]
    for f in frames:
        p = capi.Pyramid(W, H, 1)
        keep.append(p)
        p.set_level(0, f.pixelinfo)
        p.set_semantics(s, np.kron(rng.integers(0, 6, (H // 8, W // 8)), np.ones((8, 8))).astype(np.uint8))
        w.push_frame(f.frame_id, f.timestamp, None, None, win.scene.intrinsics, syn.mat_to_params(f.T_w_c_init), f.exposure, f.affine_init, f.fixed, False,
                     pyramid=p)
        w.set_landmarks(f.frame_id, f.uv[:100], f.idepth_init[:100], f.patch[:100], np.zeros(100, dtype=np.uint8))
    for r in frames:
        for t in frames:
            if r is not t:
                w.set_connection(r.frame_id, t.frame_id, np.zeros(100, dtype=np.uint8))
    m = capi.Map()
    models = {}
    for f in frames:
        m.add_keyframe(w, f.frame_id)
        models[f.frame_id] = pc.Keyframe(f.frame_id, win.scene.intrinsics.copy(), w.get_pose(f.frame_id)[0])
    w.solve()
    m.update(w)
    _model_update(models, w, win, {})
    _check_records(m, models)
    assert all(not k.type.any() for k in models.values())   # no observation yet
    w.add_semantic_observations([1])
    w.add_semantic_observations([1, 2])
    hists = {f.frame_id: w.get_semantic_observations(f.frame_id) for f in frames}
    assert hists[1].any() and hists[2].any()
    m.update(w)
    _model_update(models, w, win, {}, hists=hists)
    _check_records(m, models)
    assert models[1].type.any() and _same(models[1].type, w.get_semantic_types(1))
    weights = np.zeros(256, dtype=np.uint64)
    weights[:6] = [1, 50, 2, 900, 3, 7]
    m.update(w, weights)
    _model_update(models, w, win, {}, hists=hists, weights=weights)
    _check_records(m, models)
    assert _same(models[1].type, w.get_semantic_types(1, weights)) and not _same(models[1].type, w.get_semantic_types(1))
    check_export(m, [models[i] for i in m.keyframe_ids()], classes=pc.CLASS_ALL, colours=pc.COLOURS_SEMANTIC)
    for h in [m, w] + keep[1:] + [s]:
        h.close()


def test_refusals(tiny_window):
    from dsopp_amd import capi
    lib = capi.lib()
    win = tiny_window
    w = syn.load_window(capi.HipWindow(capi.default_pba_options()), win)
    m = capi.Map()
    code = lambda e: f"error {e}:"  # noqa: E731
    with pytest.raises(capi.HipError, match=code(ERR_NOT_FOUND)):
        m.add_keyframe(w, 77)                      # a frame the window does not hold
    m.add_keyframe(w, 0)
    with pytest.raises(capi.HipError, match=code(ERR_STATE)):
        m.add_keyframe(w, 0)                       # a second add of a live id
    with pytest.raises(capi.HipError, match=code(ERR_STATE)):
        m.set_records(0, np.ones(4), np.array([0, 0, 0, 1.0, 0, 0, 0]), np.zeros((0, 2)), np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0, np.uint8))
    for call in (lambda: m.num_records(5), lambda: m.records(5), lambda: m.export([0, 5]), lambda: m.set_pose(5, np.zeros(7))):
        with pytest.raises(capi.HipError, match=code(ERR_NOT_FOUND)):
            call()
    assert m.export_raw(m.export_options(), [0, 5], 10, {})[0] == ERR_NOT_FOUND
    # a window group, and a landmark shard of one
    g = capi.HipWindowGroup(capi.default_pba_options(), devices=[0, 0], transport=capi.TRANSPORT_LOCAL)
    syn.load_window(g, win)
    with pytest.raises(capi.HipError, match=code(ERR_INVALID_ARGUMENT)):
        m.add_keyframe(g, 1)
    with pytest.raises(capi.HipError, match=code(ERR_INVALID_ARGUMENT)):
        m.update(g)
    shard, dev = C.c_void_p(), C.c_int32()
    capi._chk(lib.dsopp_hip_window_group_shard(g._h, 0, C.byref(shard), C.byref(dev)))
    assert lib.dsopp_hip_map_add_keyframe(m._h, shard, 1, None) == ERR_INVALID_ARGUMENT
    assert lib.dsopp_hip_map_update(m._h, shard, None) == ERR_INVALID_ARGUMENT
    g.close()
    # n < 0, bad enums, null handles
    one = np.ones(4)
    T = np.array([0, 0, 0, 1.0, 0, 0, 0])
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.dsopp_hip_map_set_records(m._h, 9, ptr(one), ptr(T), -1, None, None, None, None, None, None, None) == ERR_INVALID_ARGUMENT
    assert lib.dsopp_hip_map_set_records(m._h, 9, ptr(one), ptr(T), 1, None, None, None, None, None, None, None) == ERR_INVALID_ARGUMENT
    bad_flag = np.array([4], dtype=np.uint8)
    assert lib.dsopp_hip_map_set_records(m._h, 9, ptr(one), ptr(T), 1, ptr(np.zeros(2)), ptr(one), ptr(one), ptr(one), ptr(bad_flag), None,
                                         None) == ERR_INVALID_ARGUMENT
    assert m.keyframe_ids() == [0]   # none of them left a keyframe behind
    for bad in (dict(classes=8), dict(classes=-1), dict(frame=2), dict(colours=4), dict(colours=-1)):
        rc, _ = m.export_raw(m.export_options(**bad), None, 0, {})
        assert rc == ERR_INVALID_ARGUMENT, bad
    assert m.export_raw(m.export_options(), None, -1, {})[0] == ERR_INVALID_ARGUMENT
    assert m.export_raw(None, None, 0, {})[0] == ERR_INVALID_ARGUMENT
    assert lib.dsopp_hip_map_update(None, w._h, None) == ERR_INVALID_ARGUMENT
    assert lib.dsopp_hip_map_update(m._h, None, None) == ERR_INVALID_ARGUMENT
    assert lib.dsopp_hip_map_create(0, None, None, None) == ERR_INVALID_ARGUMENT
    h = C.c_void_p()
    assert lib.dsopp_hip_map_create(capi.device_count(), None, None, C.byref(h)) == ERR_INVALID_ARGUMENT
    assert lib.dsopp_hip_map_create(0, None, C.byref(capi.default_map_options(channels=0)), C.byref(h)) == ERR_INVALID_ARGUMENT
    # the map still works
    m.update(w)
    assert m.num_records(0) == w.num_landmarks(0)
    m.close()
    w.close()


def test_example_driver_equals_the_binding(tmp_path):
    """example_point_cloud.cpp drives HipMap over the C-ABI alone — push, solve, update, choose, update, push: the same bytes as the Python
    binding composed the same way"""
    import struct
    import subprocess
    from dsopp_amd import capi
    from test_point_cloud_model import build_example
    r = subprocess.run([build_example(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr

    W, H, F, N, STEP, Z, FX = 64, 48, 5, 65, 3, 4.0, 45.0
    tri = lambda x, p: (x % (2 * p)) if (x % (2 * p)) < p else 2 * p - (x % (2 * p))  # noqa: E731
    tex = lambda x, y: 40 + 3 * tri(x, 17) + 2 * tri(y, 13) + 4 * tri(x + y, 7)  # noqa: E731
    px, py = [0, -1, 1, -2, 0, 2, -1, 0], [2, 1, 1, 0, 0, 0, -1, -2]
    lib = capi.lib()
    w = capi.HipWindow(capi.default_pba_options(function_tolerance=1e-8, parameter_tolerance=1e-8))
    w.set_deterministic(True)
    m = capi.Map(min_relative_baseline=0.05)
    intr = np.array([FX, FX, 32.0, 24.0])
    uv = np.array([[8 + (k * 7) % (W - 16), 8 + (k * 5) % (H - 16)] for k in range(N)], dtype=np.float64)
    flags = {i: np.zeros(N, dtype=np.uint8) for i in range(F)}
    statuses = {i: [] for i in range(F)}   # the targets of a frame's connections, in the order a std::map walks them
    gone, pyramids = set(), []
    ok = np.zeros(N, dtype=np.uint8)

    def connect(r_, t):
        rc = lib.dsopp_hip_window_set_connection(w._h, r_, t, N, ok.ctypes.data_as(C.c_void_p))
        assert rc in (0, ERR_NOT_FOUND), rc

    def push(i):
        t = np.array([[tex(u + STEP * i, v) for u in range(W)] for v in range(H)])
        p = capi.Pyramid(W, H, 1)
        pyramids.append(p)
        p.build_colour(None, None, np.stack([t, t + 10, t + 20], axis=2).astype(np.uint8), keep_colour=True)
        patch = np.array([[tex(int(u) + px[q] + STEP * i, int(v) + py[q]) + 10 for q in range(8)] for u, v in uv], dtype=np.float64)
        for j in range(i):
            if j not in gone:
                statuses[i].append(j)
                statuses[j].append(i)
        w.push_frame(i, 1000 * (i + 1), None, None, intr, np.array([0, 0, 0, 1, i * (STEP * (Z / FX)), 0, 0]), 1.0, np.zeros(2), i == 0, False, pyramid=p)
        w.set_landmarks(i, uv, np.full(N, 1.0 / Z), patch, flags[i])
        for j in sorted(statuses[i]):
            connect(i, j)
        for j in range(i):   # updateLocalFrame of the earlier keyframes: the flags again, every connection again
            if j in gone:
                continue
            w.set_landmarks(j, uv, np.full(N, 1.0 / Z), patch, flags[j])
            for k in sorted(statuses[j]):
                connect(j, k)
        m.add_keyframe(w, i, p)

    for i in range(F - 1):
        push(i)
    w.solve()
    m.update(w)
    got = w.choose_marginalization(capi.default_marginalization_options(strategy=mm.MAXIMUM_SIZE, maximum_size=3), apply=True)
    for fid, new in got["flags"].items():
        flags[fid] = (new & 1) | ((flags[fid] | new) & 2)
    gone.update(got["marginalized_ids"])
    m.update(w)
    push(F - 1)
    w.solve()
    m.update(w)
    c = m.export(classes=pc.CLASS_ALL, colours=pc.COLOURS_IMAGE)
    bits = lambda x: "%016x" % struct.unpack("<Q", struct.pack("<d", float(x)))[0]  # noqa: E731
    lines = ["marginalised" + "".join(f" {i}" for i in got["marginalized_ids"]) + "; keyframes" +
             "".join(f" {i}:{m.num_records(i)}" for i in m.keyframe_ids()) + f"; points {c['count']}; per keyframe" +
             "".join(f" {n}" for n in c["per_keyframe_counts"])]
    for i in range(c["count"]):
        x, y, z = c["xyz"][i]
        r_, g, b = c["rgb"][i]
        lines.append(f"{c['keyframe_index'][i]} {c['record_index'][i]} {bits(x)} {bits(y)} {bits(z)} {r_} {g} {b} {c['type'][i]} "
                     f"{bits(c['relative_baseline'][i])} {bits(c['idepth_variance'][i])}")
    active = m.export([F - 1], classes=pc.CLASS_ACTIVE, frame=pc.FRAME_KEYFRAME)["count"]
    lines.append(f"viewer: {active} active points of keyframe {F - 1}, {active} colours, {active} default colours, {active} semantic colours")
    print(r.stdout[:600])
    assert c["count"] > 100 and got["marginalized_ids"] == [0]
    assert r.stdout.strip().split("\n") == lines
    for h in [m, w] + pyramids:
        h.close()
