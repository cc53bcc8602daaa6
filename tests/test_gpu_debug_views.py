"""The tracker's debug views on the device (debug_views.hip, dsopp_hip_debug_views_*) against the NumPy statement of
tests/debug_views_model.py: images byte for byte, the state M bit for bit — the arithmetic is stated operation by operation, so there is
no tolerance anywhere.  Sizes are the smallest at which these kernels can go wrong: widths that are no multiple of 4 (a store group then
wraps into the next row) or of the 64 x 16 tile, more than one tile and more than one 4096-cell chunk, more than 256 chunks (1042 x 1009:
the closing workgroup's second round, which every 1280 x 1024 map takes), cells on every border, every pair arrangement within two radii."""
import ctypes as C
import struct

import numpy as np
import pytest

import debug_views_model as dv
import depth_maps_model as dm

pytestmark = pytest.mark.gpu

ERR_INVALID_ARGUMENT = -1
GUARD = 0xA5


def _bits(x):
    return struct.pack("<d", float(x))


def _grey3(g):
    return np.repeat(np.asarray(g)[..., None], 3, axis=2)


def _identity(capi, W, H):
    return capi.Undistorter((W, H), (W, H))


# ---- frame view

@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("size", [(77, 59), (131, 37)], ids=["77x59", "131x37"])
def test_frame_view(size, dtype):
    """masks none, random and all zero; the host-out form with a given image, the same with the image the pyramid keeps, and the
    device-out form between torch buffers (bytes behind the output untouched)"""
    import torch
    from dsopp_amd import capi
    W, H = size
    grey = dv.grey_image(W, H)
    assert {0, 127, 128, 255} <= set(grey.reshape(-1).tolist())
    rng = np.random.default_rng(W)
    masks = {"none": None, "random": (rng.random((H, W)) < 0.5).astype(np.uint8) * rng.integers(1, 256, (H, W)).astype(np.uint8),
             "zero": np.zeros((H, W), dtype=np.uint8)}
    assert 0 < (masks["random"] == 0).sum() < W * H
    v = capi.DebugViews(W, H)
    pyr = capi.Pyramid(W, H, 1, capi.F64 if dtype == "f64" else capi.F32)
    und = _identity(capi, W, H)
    stream = torch.cuda.Stream()
    d_grey = torch.from_numpy(grey.reshape(-1).copy()).cuda()
    try:
        for name, mask in masks.items():
            want = dv.frame_view(grey, mask)
            pyr.build(np.zeros((H, W), dtype=np.uint8))          # the pyramid keeps no image now
            pyr.set_mask(0, mask)
            assert pyr.get_image(1) is None
            given = v.frame(pyr, grey)
            assert given.tobytes() == want.tobytes(), (name, "grey_host")
            pyr.build_undistorted(und, grey)
            pyr.set_mask(0, mask)
            assert np.array_equal(pyr.get_image(1), grey)
            kept = v.frame(pyr)
            assert kept.tobytes() == want.tobytes(), (name, "kept image")
            d_out = torch.full((3 * W * H + 8,), GUARD, dtype=torch.uint8, device="cuda")
            d_mask = None if mask is None else torch.from_numpy(mask.reshape(-1).copy()).cuda()
            torch.cuda.synchronize()
            v.frame_device(d_grey.data_ptr(), None if mask is None else d_mask.data_ptr(), d_out.data_ptr(), stream.cuda_stream)
            stream.synchronize()
            got = d_out.cpu().numpy()
            assert got[:3 * W * H].tobytes() == want.tobytes() and (got[3 * W * H:] == GUARD).all(), (name, "device")
        assert not np.array_equal(dv.frame_view(grey, masks["zero"]), _grey3(grey))
    finally:
        for obj in (v, pyr, und):
            obj.close()


# ---- keyframe view from exact and random planes

@pytest.mark.parametrize("name", list(dv.CASES))
def test_keyframe_view_from_planes(name):
    """from M = 0 and again with the M that left (the second call smooths): image, M and cells equal the model's"""
    from dsopp_amd import capi
    c = dv.case(name)
    ids, wgt = c["planes"]
    v = capi.DebugViews(c["W"], c["H"])
    try:
        M = 0.0
        for call in range(2):
            want, M, cells = dv.keyframe_view(c["grey"], ids, wgt, M)
            got, gM, gcells = v.keyframe_planes(c["grey"], ids, wgt)
            print(f"{name} call {call}: {gcells} cells, M {gM!r} (model {M!r}), {(got != want).any(axis=2).sum()} pixels differ")
            assert gcells == cells == c["cells"]
            assert _bits(gM) == _bits(M) and _bits(v.maximum_idepth) == _bits(M)
            assert got.tobytes() == want.tobytes()
        assert (want != _grey3(c["grey"])).any()
    finally:
        v.close()


def test_ties_round_to_even_and_the_range_clamps():
    """what the model's tie and range cases hold (asserted from the model in tests/test_debug_views_model.py) shows in the device's image:
    the pixel of a cell carries colormap[level] with the level rounded half to even, 255 above M, 0 for a tiny or negative q"""
    from dsopp_amd import capi
    cm = dv.default_colormap()
    for name in ("ties", "range"):
        c = dv.case(name)
        ids, wgt = c["planes"]
        v = capi.DebugViews(c["W"], c["H"])
        try:
            got, M, _ = v.keyframe_planes(c["grey"], ids, wgt)
        finally:
            v.close()
        ok, u = dv.unrounded_levels(ids, wgt, M)
        lv = dv.levels(ids, wgt, M)
        if name == "ties":
            exact = ok & (u % 1.0 == 0.5) & (u < 255)
            k = np.floor(u[exact]).astype(int)
            assert exact.sum() >= 8 and (k % 2 == 0).any() and (k % 2 == 1).any()
            assert np.array_equal(lv.reshape(-1)[exact], k + (k & 1))
        else:
            assert sorted(lv[lv != dv.EMPTY].tolist()) == [0, 0, 0, 255]
        for y, x in zip(*np.nonzero(lv != dv.EMPTY)):
            assert tuple(got[y, x]) == tuple(cm[lv[y, x]]), (name, x, y)


def test_empty_map_and_state_sequence():
    """an empty map gives the grey view, cells = 0 and leaves M alone (0 and a set value); then a first call from M = 0 and three more
    with other maps: M equals the model's bits after each; set to 0 starts over"""
    from dsopp_amd import capi
    W, H = 77, 59
    grey = dv.grey_image(W, H, seed=3)
    zero = np.zeros((H, W))
    v = capi.DebugViews(W, H)
    try:
        for preset in (0.0, 3.5):
            v.maximum_idepth = preset
            got, M, cells = v.keyframe_planes(grey, zero, zero)
            assert cells == 0 and _bits(M) == _bits(preset) and _bits(v.maximum_idepth) == _bits(preset)
            assert got.tobytes() == _grey3(grey).tobytes()
        v.maximum_idepth = 0.0
        M, seen = 0.0, []
        for call in range(4):
            c = dv._random(W, H, 0.02 * (call + 1), seed=200 + call)
            ids, wgt = c["planes"]
            ids = ids * (1.0 + call)          # another average every call, so that M moves
            want, M, cells = dv.keyframe_view(grey, ids, wgt, M)
            got, gM, gcells = v.keyframe_planes(grey, ids, wgt)
            assert gcells == cells and _bits(gM) == _bits(M), (call, gM, M)
            assert got.tobytes() == want.tobytes(), call
            seen.append(M)
        assert len(set(seen)) == 4
        v.maximum_idepth = 0.0
        c = dv._random(W, H, 0.02, seed=200)
        want, M0, _ = dv.keyframe_view(grey, *c["planes"], 0.0)
        got, gM, _ = v.keyframe_planes(grey, *c["planes"])
        assert _bits(gM) == _bits(M0) == _bits(seen[0]) and got.tobytes() == want.tobytes()
    finally:
        v.close()


@pytest.mark.parametrize("name", ["clipping", "pairs", "300x41_50pct"])
def test_custom_colormap_and_asymmetric_stencil(name):
    """the stencil's orientation: byte (dy + 3, dx + 3) set means the circle at c covers c + (dx, dy)"""
    from dsopp_amd import capi
    c = dv.case(name)
    ids, wgt = c["planes"]
    colormap, stencil = dv.custom_colormap(), dv.asymmetric_stencil()
    want, M, cells = dv.keyframe_view(c["grey"], ids, wgt, 0.0, colormap, stencil)
    assert want.tobytes() != dv.keyframe_view(c["grey"], ids, wgt, 0.0, colormap, stencil[::-1, ::-1])[0].tobytes()
    assert want.tobytes() != dv.keyframe_view(c["grey"], ids, wgt, 0.0, colormap, stencil.T)[0].tobytes()
    for cm_arg, st_arg in ((colormap, stencil), (colormap, None), (None, stencil)):
        v = capi.DebugViews(c["W"], c["H"], cm_arg, st_arg)
        try:
            got, gM, gcells = v.keyframe_planes(c["grey"], ids, wgt)
        finally:
            v.close()
        assert gcells == cells and _bits(gM) == _bits(M)
        assert got.tobytes() == dv.keyframe_view(c["grey"], ids, wgt, 0.0, cm_arg, st_arg)[0].tobytes(), (cm_arg is None, st_arg is None)


# ---- keyframe view from device-resident maps

@pytest.mark.parametrize("name", ["edges", "sparse", "general_const"])
def test_keyframe_view_from_device_maps(name):
    """windows loaded, not solved, as tests/test_gpu_depth_map_edges.py loads them: the maps form (kept image and given image), its
    device-out form and the planes form fed the planes get_level(0) returns give identical bytes and identical M, the model's"""
    import torch
    from dsopp_amd import capi
    import test_gpu_depth_map_edges as edges
    c = dm.case(name)
    W, H = c["W"], c["H"]
    grey = dv.grey_image(W, H, seed=9)
    g = edges._load(c, capi)
    maps = g.create_reference_depth_maps(c["levels"])
    ids, wgt = maps.get_level(0)
    assert (ids > 0).sum() > 10
    want, M, cells = dv.keyframe_view(grey, ids, wgt, 0.0)
    v = capi.DebugViews(W, H)
    pyr = capi.Pyramid(W, H, 1)
    und = _identity(capi, W, H)
    try:
        pyr.build_undistorted(und, grey)
        results = {"maps, kept image": v.keyframe(pyr, maps)}
        v.maximum_idepth = 0.0
        results["maps, given image"] = v.keyframe(pyr, maps, grey)
        v.maximum_idepth = 0.0
        results["planes"] = v.keyframe_planes(grey, ids, wgt)
        v.maximum_idepth = 0.0
        stream = torch.cuda.Stream()
        d_grey = torch.from_numpy(grey.reshape(-1).copy()).cuda()
        d_out = torch.full((3 * W * H + 8,), GUARD, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        v.keyframe_device(d_grey.data_ptr(), maps, d_out.data_ptr(), stream.cuda_stream)
        M_dev = v.maximum_idepth            # (waits for the two launches)
        stream.synchronize()
        out = d_out.cpu().numpy()
        assert (out[3 * W * H:] == GUARD).all()
        results["maps, device out"] = (out[:3 * W * H].reshape(H, W, 3), M_dev, cells)
        for what, (img, gM, gcells) in results.items():
            print(f"{name} {what}: {gcells} cells, M {gM!r} (model {M!r})")
            assert gcells == cells and _bits(gM) == _bits(M), what
            assert img.tobytes() == want.tobytes(), what
        # the planes are where they were: the maps are read, never written
        again = maps.get_level(0)
        assert again[0].tobytes() == ids.tobytes() and again[1].tobytes() == wgt.tobytes()
    finally:
        for obj in (v, pyr, und, maps, g):
            obj.close()


# ---- errors

def test_errors():
    from dsopp_amd import capi
    lib = capi.lib()
    W, H = 77, 59
    grey = dv.grey_image(W, H)
    out = np.zeros((H, W, 3), dtype=np.uint8)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)                 # noqa: E731
    h = C.c_void_p()
    bad = dv.default_stencil()
    bad[3, 3] = 0
    assert lib.dsopp_hip_debug_views_create(0, None, W, H, None, ptr(bad), C.byref(h)) == ERR_INVALID_ARGUMENT
    assert lib.dsopp_hip_debug_views_create(0, None, W, H, None, None, None) == ERR_INVALID_ARGUMENT
    assert lib.dsopp_hip_debug_views_create(0, None, 0, H, None, None, C.byref(h)) == ERR_INVALID_ARGUMENT
    assert lib.dsopp_hip_debug_views_create(capi.device_count(), None, W, H, None, None, C.byref(h)) == ERR_INVALID_ARGUMENT
    v = capi.DebugViews(W, H)
    pyr, other = capi.Pyramid(W, H, 1), capi.Pyramid(W + 1, H, 1)
    c = dm.case("sparse")                                         # 131 x 37: another size than the views
    import test_gpu_depth_map_edges as edges
    g = edges._load(c, capi)
    maps = g.create_reference_depth_maps(1)
    c77 = dm.case("edges")
    g77 = edges._load(c77, capi)
    maps77 = g77.create_reference_depth_maps(1)
    M, cells = C.c_double(), C.c_int64()
    try:
        calls = {
            "frame: null views": lambda: lib.dsopp_hip_debug_views_frame(None, pyr._h, ptr(grey), ptr(out)),
            "frame: null pyramid": lambda: lib.dsopp_hip_debug_views_frame(v._h, None, ptr(grey), ptr(out)),
            "frame: null output": lambda: lib.dsopp_hip_debug_views_frame(v._h, pyr._h, ptr(grey), None),
            "frame: another size": lambda: lib.dsopp_hip_debug_views_frame(v._h, other._h, ptr(grey), ptr(out)),
            "frame: no kept image": lambda: lib.dsopp_hip_debug_views_frame(v._h, pyr._h, None, ptr(out)),
            "frame_device: null image": lambda: lib.dsopp_hip_debug_views_frame_device(v._h, None, None, C.c_void_p(4096), None),
            "frame_device: null output": lambda: lib.dsopp_hip_debug_views_frame_device(v._h, C.c_void_p(4096), None, None, None),
            "frame_device: unaligned output": lambda: lib.dsopp_hip_debug_views_frame_device(v._h, C.c_void_p(4096), None, C.c_void_p(4098), None),
            "keyframe: null views": lambda: lib.dsopp_hip_debug_views_keyframe(None, pyr._h, ptr(grey), maps77._h, ptr(out), C.byref(M), C.byref(cells)),
            "keyframe: null maps": lambda: lib.dsopp_hip_debug_views_keyframe(v._h, pyr._h, ptr(grey), None, ptr(out), C.byref(M), C.byref(cells)),
            "keyframe: null pyramid": lambda: lib.dsopp_hip_debug_views_keyframe(v._h, None, ptr(grey), maps77._h, ptr(out), C.byref(M), C.byref(cells)),
            "keyframe: null output": lambda: lib.dsopp_hip_debug_views_keyframe(v._h, pyr._h, ptr(grey), maps77._h, None, C.byref(M), C.byref(cells)),
            "keyframe: maps of another size": lambda: lib.dsopp_hip_debug_views_keyframe(v._h, pyr._h, ptr(grey), maps._h, ptr(out), C.byref(M), C.byref(cells)),
            "keyframe: pyramid of another size": lambda: lib.dsopp_hip_debug_views_keyframe(v._h, other._h, ptr(grey), maps77._h, ptr(out), C.byref(M), C.byref(cells)),
            "keyframe: no kept image": lambda: lib.dsopp_hip_debug_views_keyframe(v._h, pyr._h, None, maps77._h, ptr(out), C.byref(M), C.byref(cells)),
            "keyframe_device: null maps": lambda: lib.dsopp_hip_debug_views_keyframe_device(v._h, C.c_void_p(4096), None, C.c_void_p(4096), None),
            "keyframe_device: maps of another size": lambda: lib.dsopp_hip_debug_views_keyframe_device(v._h, C.c_void_p(4096), maps._h, C.c_void_p(4096), None),
            "keyframe_device: unaligned output": lambda: lib.dsopp_hip_debug_views_keyframe_device(v._h, C.c_void_p(4096), maps77._h, C.c_void_p(4097), None),
            "keyframe_planes: null plane": lambda: lib.dsopp_hip_debug_views_keyframe_planes(v._h, ptr(grey), None, None, ptr(out), C.byref(M), C.byref(cells)),
            "keyframe_planes: null image": lambda: lib.dsopp_hip_debug_views_keyframe_planes(v._h, None, ptr(np.zeros((H, W))), ptr(np.zeros((H, W))), ptr(out), C.byref(M), C.byref(cells)),
            "get: null": lambda: lib.dsopp_hip_debug_views_get_maximum_idepth(v._h, None),
            "set: null": lambda: lib.dsopp_hip_debug_views_set_maximum_idepth(None, C.c_double(1.0)),
        }
        for what, call in calls.items():
            assert call() == ERR_INVALID_ARGUMENT, what
        if capi.device_count() > 1:                               # handles on different devices
            far = capi.Pyramid(W, H, 1, device=1)
            try:
                assert lib.dsopp_hip_debug_views_frame(v._h, far._h, ptr(grey), ptr(out)) == ERR_INVALID_ARGUMENT
            finally:
                far.close()
        # none of the refused calls touched the state, and the object still works: the matching maps, with the image given
        assert v.maximum_idepth == 0.0
        img, gM, gcells = v.keyframe(pyr, maps77, grey)
        ids, wgt = maps77.get_level(0)
        want, wM, wcells = dv.keyframe_view(grey, ids, wgt, 0.0)
        assert img.tobytes() == want.tobytes() and _bits(gM) == _bits(wM) and gcells == wcells
    finally:
        for obj in (v, pyr, other, maps, g, maps77, g77):
            obj.close()
