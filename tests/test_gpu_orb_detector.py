"""The device ORB keypoint detector (dsopp_hip_orb_detector, dsopp_amd/csrc/orb.hip) against tests/orb_model.py: level images, mask
bytes, FAST score planes, n, xy, level and response bit for bit — every step is an integer or a single stated float operation, so there
is nothing to tolerate and no point is left out."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import optical_flow_model as ofm
import orb_model as om
import test_orb_detector as tod

pytestmark = pytest.mark.gpu

# (width, height, edge_threshold, nlevels, nfeatures, cell of the texture): odd sizes whose halvings round half to even, a size whose last
# levels are too small for the border, and the reference's constants
CONFIGS = {
    "160x120": (160, 120, 8, 3, 60, 8),
    "163x121": (163, 121, 8, 3, 60, 8),
    "64x64": (64, 64, 8, 2, 8, 8),
    "100x80": (100, 80, 31, 3, 12, 8),
    "640x480": (640, 480, 31, 5, 500, 16),
}
MASKS = ["none", "band", "random", "ones"]
GUARD = 0x5A


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _mask(kind, width, height):
    """None, a masked band, 15 % random masked pixels, or bytes of value 1 (valid at level 0, masked above) over the left half"""
    if kind == "none":
        return None
    m = np.full((height, width), 255, np.uint8)
    if kind == "band":
        m[height // 3:height // 2, :] = 0
    elif kind == "random":
        m[np.random.default_rng(width).random((height, width)) < 0.15] = 0
    else:
        m[:, :width // 2] = 1
    return m


@functools.lru_cache(maxsize=None)
def _texture(name):
    w, h, _, _, _, cell = CONFIGS[name]
    img = tod.texture(w, h, cell=cell)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _model(name, mask_kind, nfeatures=None):
    w, h, e, levels, nf, _ = CONFIGS[name]
    return om.detect(_texture(name), _mask(mask_kind, w, h), nf if nfeatures is None else nfeatures, levels, e, 20)


def _detector(name, nfeatures=None):
    from dsopp_amd import capi
    w, h, e, levels, nf, _ = CONFIGS[name]
    return capi.OrbDetector(w, h, nf if nfeatures is None else nfeatures, levels, e, 20)


def _assert_detection(got, want, what=""):
    xy, level, response = got
    assert len(level) == len(want.level), f"{what}: {len(level)} detections, the model has {len(want.level)}"
    assert np.array_equal(level, want.level), what
    assert np.array_equal(_bits(xy), _bits(want.xy)), f"{what}: positions differ first at {np.argwhere(_bits(xy) != _bits(want.xy))[:3]}"
    assert np.array_equal(_bits(response), _bits(want.response)), f"{what}: responses differ first at {np.argwhere(_bits(response) != _bits(want.response))[:3]}"


def _assert_planes(det, want, what=""):
    for l in range(det.num_levels):
        image, mask, score = det.get_level(l)
        assert np.array_equal(image, want.images[l]), f"{what}: image of level {l}"
        assert np.array_equal(score, want.scores[l]), f"{what}: score plane of level {l} differs at {np.argwhere(score != want.scores[l])[:3]}"
        assert np.array_equal(mask, want.masks[l] if want.masks is not None else np.full_like(image, 255)), f"{what}: mask of level {l}"


@pytest.mark.parametrize("name", ["160x120", "640x480"])
def test_both_cuts_bite_on_every_level_of_the_texture(name):
    """the condition the texture is chosen for, asserted on the model: on every level that has an interior more survivors than
    2 n_l, and more than n_l behind the first cut"""
    w, h, e, levels, nf, _ = CONFIGS[name]
    d = _model(name, "none")
    per_level = om.features_per_level(nf, levels)
    with_interior = [l for l in range(levels) if min(om.level_size(w, h, l)) > 2 * e]
    assert len(with_interior) == 3
    for l in with_interior:
        assert len(d.filtered[l][0]) > 2 * per_level[l] > 0 and len(d.first_cut[l][0]) > per_level[l] and len(d.final[l][0]) >= per_level[l]
        assert 2 * per_level[l] <= len(d.first_cut[l][0]) < len(d.filtered[l][0])
    for l in range(levels):
        if l not in with_interior:
            assert len(d.filtered[l][0]) == 0


@pytest.mark.parametrize("mask_kind", MASKS)
@pytest.mark.parametrize("name", list(CONFIGS))
def test_texture_from_a_host_image(name, mask_kind):
    w, h = CONFIGS[name][:2]
    want = _model(name, mask_kind)
    assert len(want.level) > 0
    det = _detector(name)
    det.set_mask(_mask(mask_kind, w, h))
    _assert_detection(det.detect(_texture(name)), want, "dense")
    _assert_planes(det, want)
    wide = np.full((h, w + 7), GUARD, np.uint8)                                 # a host image with a row stride of its own
    wide[:, :w] = _texture(name)
    _assert_detection(det.detect(wide[:, :w]), want, "strided")
    det.set_mask(None)                                                          # and the mask can be taken away again
    _assert_detection(det.detect(_texture(name)), _model(name, "none"), "mask removed")
    det.close()


def test_flat_image_gives_nothing():
    det = _detector("160x120")
    xy, level, response = det.detect(np.full((120, 160), 93, np.uint8))
    assert len(level) == 0 and xy.shape == (0, 2)
    for l in range(3):
        assert not det.get_level(l)[2].any()
    det.close()


def _hand_dots():
    """dots at x = e - 1, e, w - e - 1, w - e and the same in y, one on a masked pixel, one beside a masked stronger corner"""
    w, h, e = 96, 64, 8
    points = [(e - 1, 20, 200), (e, 30, 200), (w - e - 1, 20, 190), (w - e, 30, 200), (30, e - 1, 200), (40, e, 180), (30, h - e - 1, 170), (40, h - e, 200),
              (50, 32, 200), (70, 40, 200), (71, 40, 180), (20, 45, 160)]
    mask = np.full((h, w), 255, np.uint8)
    mask[32, 50] = 0
    mask[40, 70] = 0
    return tod.dots(w, h, points), mask, e


def test_hand_placed_dots_at_the_border_and_the_mask():
    from dsopp_amd import capi
    img, mask, e = _hand_dots()
    want = om.detect(img, mask, 100, 1, e, 20)
    assert sorted(map(tuple, want.xy.tolist())) == sorted([(8.0, 30.0), (87.0, 20.0), (40.0, 8.0), (30.0, 55.0), (20.0, 45.0)])
    det = capi.OrbDetector(96, 64, 100, 1, e, 20)
    det.set_mask(mask)
    _assert_detection(det.detect(img), want)
    _assert_planes(det, want)
    det.close()
    # the ties of tests/test_orb_detector.py: both cuts keep their tied group whole
    for values, kept in (([170, 140, 160, 140, 120, 140, 150], 2), ([150, 180, 150, 110, 150], 4)):
        tie = tod.tie_dots(values)
        want = om.detect(tie, None, 2, 1, 8, 20)
        assert len(want.level) == kept
        det = capi.OrbDetector(tie.shape[1], tie.shape[0], 2, 1, 8, 20)
        _assert_detection(det.detect(tie), want, f"ties {values}")
        det.close()
    # identical dots all over: every survivor ties at both cuts and all of them come back, far more than nfeatures and than the
    # nfeatures + 256 records that return with the header
    many = tod.dots(320, 240, [(x, y, 200) for y in range(10, 232, 10) for x in range(10, 312, 10)])
    want = om.detect(many, None, 4, 1, 8, 20)
    assert len(want.level) == 23 * 31
    det = capi.OrbDetector(320, 240, 4, 1, 8, 20)
    _assert_detection(det.detect(many), want, "all tied")
    det.close()


@pytest.mark.parametrize("nfeatures", [0, 1, 100000])
def test_nfeatures_none_one_and_more_than_there_are(nfeatures):
    want = _model("160x120", "none", nfeatures)
    if nfeatures == 0:
        assert len(want.level) == 0
    if nfeatures == 1:
        assert want.level.tolist() == [0]
    if nfeatures == 100000:
        assert [len(f[0]) for f in want.final] == [len(f[0]) for f in want.filtered]
    det = _detector("160x120", nfeatures)
    _assert_detection(det.detect(_texture("160x120")), want)
    det.close()


@pytest.mark.parametrize("nfeatures", [3000, 100000])
def test_lists_longer_than_the_selecting_workgroup(nfeatures):
    """640 x 480 with 8-pixel cells: several thousand survivors on level 0, so the second cut selects among, and the output is compacted
    from, more entries than the one workgroup that does both has threads (1024) — with the cut biting (3000) and keeping all (100000)"""
    from dsopp_amd import capi
    img = tod.texture(640, 480, cell=8, seed=2)
    want = om.detect(img, None, nfeatures, 5, 31, 20)
    per_level = om.features_per_level(nfeatures, 5)
    assert len(want.first_cut[0][0]) > 2048 and len(want.first_cut[1][0]) > 1024
    if nfeatures == 3000:
        assert len(want.filtered[0][0]) > len(want.first_cut[0][0]) > per_level[0] == len(want.final[0][0])
    else:
        assert len(want.final[0][0]) == len(want.filtered[0][0])
    det = capi.OrbDetector(640, 480, nfeatures, 5, 31, 20)
    _assert_detection(det.detect(img), want)
    det.close()


@pytest.mark.parametrize("name", ["163x121", "64x64"])
def test_device_pointer_with_a_stride_at_an_odd_address(name):
    import torch
    w, h = CONFIGS[name][:2]
    stride = w + 5
    host = np.full(h * stride + 1, GUARD, np.uint8)
    host[1:].reshape(h, stride)[:, :w] = _texture(name)
    buf = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    det = _detector(name)
    _assert_detection(det.detect(buf.data_ptr() + 1, stride), _model(name, "none"))
    _assert_planes(det, _model(name, "none"))
    det.close()


def test_pyramid_kept_image_and_mask_from_pyramid():
    """the grey image a pyramid keeps behind build_transformed and its level-0 mask as validity: a byte of 1 counts as 255 there"""
    from dsopp_amd import capi
    w, h, e, levels, nf, _ = CONFIGS["160x120"]
    tr = capi.Transformer((2 * w, 2 * h), resize_ratio=0.5, crop_levels=0)
    p = capi.Pyramid(w, h, 1)
    p.build_transformed(None, tr, tod.texture(2 * w, 2 * h, cell=16, seed=4))
    kept = p.get_image(1)
    assert kept is not None and kept.shape == (h, w)
    static = _mask("band", w, h)
    static[:, :w // 4] = 1
    sem = capi.Semantics(w, h, 1, static, None)
    p.set_semantics(sem, None)
    det = _detector("160x120")
    _assert_detection(det.detect(p), om.detect(kept, None, nf, levels, e, 20), "no mask")
    det.set_mask_from_pyramid(p)
    want = om.detect(kept, np.where(static != 0, 255, 0).astype(np.uint8), nf, levels, e, 20)
    _assert_detection(det.detect(p), want, "validity")
    _assert_planes(det, want)
    det.set_mask(static)                                                        # the bytes themselves: the 1s mask the levels above 0
    bytes_want = om.detect(kept, static, nf, levels, e, 20)
    assert not np.array_equal(bytes_want.masks[1], want.masks[1])
    _assert_detection(det.detect(p), bytes_want, "bytes")
    for o in (det, sem, p, tr):
        o.close()


def test_guard_bytes_capacity_and_repeats():
    name = "160x120"
    want = _model(name, "none")
    n = len(want.level)
    det = _detector(name)
    pad = 16

    def guarded(cap):
        raw = [np.full(2 * cap + 2 * pad, np.float32(-7.5), np.float32), np.full(cap + 2 * pad, -77, np.int32), np.full(cap + 2 * pad, np.float32(-7.5), np.float32)]
        views = (raw[0][pad:pad + 2 * cap].reshape(cap, 2), raw[1][pad:pad + cap], raw[2][pad:pad + cap])
        return raw, views

    # room for more than comes back: nothing is written past n or outside the arrays
    raw, views = guarded(n + 9)
    rc, got_n, xy, level, response = det.detect_raw(_texture(name), n + 9, outputs=views)
    assert rc == 0 and got_n == n
    _assert_detection((xy[:n], level[:n], response[:n]), want)
    first = [r.copy() for r in raw]
    assert np.all(raw[0][:pad] == -7.5) and np.all(raw[0][pad + 2 * n:] == -7.5)
    assert np.all(raw[1][:pad] == -77) and np.all(raw[1][pad + n:] == -77)
    assert np.all(raw[2][:pad] == -7.5) and np.all(raw[2][pad + n:] == -7.5)
    # the same call again: identical bytes
    raw2, views2 = guarded(n + 9)
    assert det.detect_raw(_texture(name), n + 9, outputs=views2)[:2] == (0, n)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, raw2))
    # exactly enough is enough; one short is DSOPP_HIP_ERR_CAPACITY with the count needed and nothing written
    raw, views = guarded(n)
    assert det.detect_raw(_texture(name), n, outputs=views)[:2] == (0, n)
    raw, views = guarded(n - 1)
    assert det.detect_raw(_texture(name), n - 1, outputs=views)[:2] == (-5, n)
    assert np.all(raw[0] == -7.5) and np.all(raw[1] == -77) and np.all(raw[2] == -7.5)
    assert det.detect_raw(_texture(name), 0)[:2] == (-5, n)
    _assert_detection(det.detect(_texture(name)), want, "after the refusals")
    det.close()


def test_two_detectors_of_different_sizes_called_alternately():
    a, b = _detector("163x121"), _detector("64x64")
    b.set_mask(_mask("random", 64, 64))
    for _ in range(3):
        _assert_detection(a.detect(_texture("163x121")), _model("163x121", "none"))
        _assert_detection(b.detect(_texture("64x64")), _model("64x64", "random"))
    a.close()
    b.close()


def test_error_codes():
    from dsopp_amd import capi
    lib = capi.lib()
    h = C.c_void_p()
    good = dict(width=64, height=48, nfeatures=10, nlevels=2, edge=8, fast=20)
    for change in (dict(nlevels=0), dict(nlevels=9), dict(edge=3), dict(fast=-1), dict(fast=256), dict(nfeatures=-1), dict(width=0), dict(height=0),
                   dict(width=1, nlevels=2), dict(height=2, nlevels=4)):
        a = dict(good, **change)
        rc = lib.dsopp_hip_orb_detector_create(a["width"], a["height"], a["nfeatures"], a["nlevels"], a["edge"], a["fast"], 0, None, C.byref(h))
        assert rc == -1, change
    assert lib.dsopp_hip_orb_detector_create(64, 48, 10, 2, 8, 20, 0, None, None) == -1
    assert lib.dsopp_hip_orb_detector_create(64, 48, 10, 2, 8, 20, 99, None, C.byref(h)) == -1      # no such device
    capi.OrbDetector(1, 1, 0, 1, 4, 0).close()                                  # the least of everything is a detector
    det = capi.OrbDetector(64, 48, 10, 2, 8, 20)
    n = C.c_int32()
    xy, level, response = np.zeros((16, 2), np.float32), np.zeros(16, np.int32), np.zeros(16, np.float32)
    out = (16, capi._p(xy, np.float32), capi._p(level, np.int32), capi._p(response, np.float32), C.byref(n))
    assert lib.dsopp_hip_orb_detector_get_level(det._h, 0, capi._p(np.zeros((48, 64), np.uint8), np.uint8), None, None, None, None) == -6   # nothing detected yet
    assert lib.dsopp_hip_orb_detector_get_level(det._h, 2, None, None, None, None, None) == -1
    assert lib.dsopp_hip_orb_detector_detect_from_pyramid(det._h, None, *out) == -1
    assert lib.dsopp_hip_orb_detector_set_mask_from_pyramid(det._h, None) == -1
    assert lib.dsopp_hip_orb_detector_detect(det._h, None, C.c_size_t(64), *out) == -1
    img = np.zeros((48, 64), np.uint8)
    assert lib.dsopp_hip_orb_detector_detect(det._h, capi._p(img, np.uint8), C.c_size_t(63), *out) == -1        # a stride below the width
    assert lib.dsopp_hip_orb_detector_detect_device(det._h, None, C.c_size_t(64), *out) == -1
    assert lib.dsopp_hip_orb_detector_detect(det._h, capi._p(img, np.uint8), C.c_size_t(64), 16, None, None, None, C.byref(n)) == -1
    assert lib.dsopp_hip_orb_detector_detect(det._h, capi._p(img, np.uint8), C.c_size_t(64), -1, *out[1:]) == -1
    other = capi.Pyramid(32, 48, 1)                                             # another size
    assert lib.dsopp_hip_orb_detector_detect_from_pyramid(det._h, other._h, *out) == -1
    assert lib.dsopp_hip_orb_detector_set_mask_from_pyramid(det._h, other._h) == -1
    plain = capi.Pyramid(64, 48, 1)                                             # the right size, but a plain build keeps no 8-bit image
    plain.build(img)
    assert lib.dsopp_hip_orb_detector_detect_from_pyramid(det._h, plain._h, *out) == -6
    assert lib.dsopp_hip_orb_detector_set_mask_from_pyramid(det._h, plain._h) == -1                     # and it never had set_semantics
    assert lib.dsopp_hip_orb_detector_detect(det._h, capi._p(img, np.uint8), C.c_size_t(64), *out) == 0 and n.value == 0
    for o in (det, other, plain):
        o.close()


def test_host_mirror_over_three_frames(tmp_path):
    """HipFindCorrespondences through its driver: the first frame's detection, then two frames matched against it with 4 features moved
    off the image — the flow loses them and the refill draws as many from the fresh detection in the shuffle order"""
    from dsopp_amd import capi
    w, h, nf, levels, e, lost = 96, 64, 30, 2, 8, 4
    big = tod.texture(w + 4, h + 4, seed=5)
    frames = [np.ascontiguousarray(big[k:k + h, k:k + w]) for k in range(3)]
    path = tmp_path / "frames.bin"
    with open(path, "wb") as f:
        f.write(f"{w} {h} 3 {nf} {levels} {e} {lost}\n".encode())
        for frame in frames:
            f.write(frame.tobytes())
    exe = tod.build_example(tmp_path)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got, lines = [], r.stdout.split("\n")
    for line in lines:
        if line.startswith("frame"):
            got.append(([], []))
        elif line.startswith("f "):
            got[-1][0].append([int(v, 16) for v in line.split()[1:]])
        elif line.startswith("c "):
            got[-1][1].append([int(v) for v in line.split()[1:]])
    assert len(got) == 3
    detections = [om.detect(frame, None, nf, levels, e, 20).xy for frame in frames]
    features, corr = om.find_correspondences(None, None, frames[0], detections[0], nf, capi.features_shuffle_order)
    assert np.array_equal(np.array(got[0][0], np.uint32).reshape(-1, 2), _bits(features)) and got[0][1] == []
    features_from = features.copy()
    for i in range(lost):
        features_from[len(features_from) - 1 - i] = (-1000.0 - i, -1000.0)
    tracker = ofm.Tracker(w, h)
    tracker.set_reference(frames[0])
    for k in (1, 2):
        features, corr = om.find_correspondences(features_from, tracker, frames[k], detections[k], nf, capi.features_shuffle_order)
        assert len(corr) <= len(features_from) - lost and len(features) == nf and len(features) - len(corr) >= lost      # a real refill
        assert np.array_equal(np.array(got[k][0], np.uint32).reshape(-1, 2), _bits(features)), f"features of frame {k}"
        assert np.array_equal(np.array(got[k][1], np.int64).reshape(-1, 2), corr), f"correspondences of frame {k}"
