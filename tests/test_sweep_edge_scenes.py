"""The scenes of tests/sweep_edge_scenes.py reach the edges they were built for — asserted on the CPU oracle alone, so a scene that stops
saying "outside" (or stops converging) fails here, on any machine, and cannot make tests/test_gpu_sweep_frame_edges.py pass by default.

Measured with the oracle (residuals OK / out of bounds of 480 after begin() + calculate_energy(); iterations of optimize()):
  border    161x121  289 / 191, 5    162x123  274 / 206, 7    163x122  277 / 203, 5    160x120  267 / 213, 5
  interior  161x121  460 /  20, 4    162x123  472 /   8, 7    163x122  472 /   8, 5    160x120  473 /   7, 7
  mixed     163x121, 160x123, 162x122   461 / 19, 5        the same keyframes as 160x123, 162x122, 163x121   463 / 17, 6
  level     1 (163 x 122)   473 / 7, 4                     2 (81 x 61)   466 / 14, 5
"""
import functools

import numpy as np
import pytest

import sweep_edge_scenes as ses


@functools.lru_cache(maxsize=None)
def _candidates(builder):
    """{(r, t): candidate statuses} of the oracle after begin() + calculate_energy()"""
    from oracle import pyoracle as po
    scene = builder()
    o = ses.load(po.OracleWindow(po.default_pba_options()), scene)
    o.begin()
    o.calculate_energy()
    out = {(r, t): o.get_residuals(r, t)["candidate"].copy() for r, t in ses.pairs(scene)}
    o.close()
    for c in out.values():
        assert np.isin(c, (ses.STATUS_OK, ses.STATUS_OOB)).all()   # nothing else can come out of the first evaluation
    return out


def _shares(cands):
    allc = np.concatenate(list(cands.values()))
    return int((allc == ses.STATUS_OK).sum()), int((allc == ses.STATUS_OOB).sum()), len(allc)


def _iterations(scene):
    from oracle import pyoracle as po
    o = ses.load(po.OracleWindow(po.default_pba_options()), scene)
    _, it, _ = o.optimize()
    o.close()
    return it


@pytest.mark.parametrize("width,height", ses.SIZES)
def test_border_scene_decides_outside_at_every_edge(width, height):
    scene = ses.border(width, height)
    cands = _candidates(functools.partial(ses.border, width, height))
    n_ok, n_oob, n = _shares(cands)
    print(f"{scene.name}: {n_ok} OK / {n_oob} out of bounds of {n}")
    assert n == 2 * ses.NUM_FRAMES * ses.PER_FRAME
    assert n_ok >= 0.25 * n and n_oob >= 0.25 * n
    # per target edge: out-of-bounds residuals whose centre reprojects beyond the ROI limit, OK ones whose centre lands within 8 pixels
    # inside it, and out-of-bounds ones that only the TARGET side can have decided (the reference pattern lies inside its ROI)
    lo = float(ses.ROI_BORDER)
    beyond, inside, target_side, on_limit = np.zeros(4, int), np.zeros(4, int), np.zeros(4, int), np.zeros(4, int)
    for (r, t), c in cands.items():
        # OK residuals of landmarks whose pattern arm (u +- 2, v +- 2) sits exactly ON a reference limit: an exclusive comparison loses them
        ur, vr = scene.window.frames[r].uv.T
        for e, at in enumerate((ur - 2 == ses.ROI_BORDER, ur + 2 == width - 5, vr - 2 == ses.ROI_BORDER, vr + 2 == height - 5)):
            on_limit[e] += int(((c == ses.STATUS_OK) & at).sum())
        tu, tv = ses.reproject_centres(scene, r, t)
        wt, ht = scene.size(t)
        wr, hr = scene.size(r)
        hi_u, hi_v = wt - ses.ROI_BORDER - 1.0, ht - ses.ROI_BORDER - 1.0
        uv = scene.window.frames[r].uv
        ref_in = (uv[:, 0] - 2 >= lo) & (uv[:, 0] + 2 <= wr - 5) & (uv[:, 1] - 2 >= lo) & (uv[:, 1] + 2 <= hr - 5)
        oob, ok = c == ses.STATUS_OOB, c == ses.STATUS_OK
        for e, (out, near, arm_out) in enumerate((
                (tu < lo, (tu >= lo) & (tu < lo + 8), tu - 2 < lo),
                (tu > hi_u, (tu <= hi_u) & (tu > hi_u - 8), tu + 2 > hi_u),
                (tv < lo, (tv >= lo) & (tv < lo + 8), tv - 2 < lo),
                (tv > hi_v, (tv <= hi_v) & (tv > hi_v - 8), tv + 2 > hi_v))):
            beyond[e] += int((oob & out).sum())
            inside[e] += int((ok & near).sum())
            target_side[e] += int((oob & ref_in & arm_out).sum())
    print(f"  per edge (left, right, top, bottom): beyond {beyond}, OK within 8 {inside}, target-side only {target_side}, on the limit {on_limit}")
    assert (beyond >= 8).all(), beyond
    assert (inside >= 8).all(), inside
    assert (target_side >= 8).all(), target_side
    assert (on_limit >= 2).all(), on_limit
    # the reference-side ROI and the first-estimate-Jacobians u +- 2 test: landmarks 2 and 3 pixels from an edge, in every keyframe
    for f in scene.window.frames:
        u, v = f.uv[:, 0], f.uv[:, 1]
        assert u.min() >= 2 and v.min() >= 2 and u.max() <= width - 3 and v.max() <= height - 3
        assert (np.isin(u, (2, 3, width - 4, width - 3)) | np.isin(v, (2, 3, height - 4, height - 3))).sum() >= 8
        edge = (u < 8) | (u > width - 9) | (v < 8) | (v > height - 9)
        assert 0.4 * len(u) <= edge.sum() <= 0.6 * len(u)    # "about half" within 8 pixels of an edge
    it = _iterations(scene)
    print(f"  {it} iterations")
    assert it >= 2


@pytest.mark.parametrize("name,builder", [s for s in ses.F64_SCENES if not s[0].startswith("border")]
                         + [("mixed-permuted", functools.partial(ses.mixed, ses.MIXED_SIZES_PERMUTED))])
def test_scene_is_mostly_inside_and_takes_more_than_one_step(name, builder):
    scene = builder()
    n_ok, n_oob, n = _shares(_candidates(builder))
    it = _iterations(scene)
    print(f"{scene.name}: {n_ok} OK / {n_oob} out of bounds of {n}, {it} iterations")
    assert n == 2 * ses.NUM_FRAMES * ses.PER_FRAME
    assert n_ok >= 0.6 * n
    assert it >= 2


def test_mixed_scene_frames_have_their_own_sizes():
    for sizes in (ses.MIXED_SIZES, ses.MIXED_SIZES_PERMUTED):
        scene = ses.mixed(sizes)
        assert tuple(scene.size(i) for i in range(ses.NUM_FRAMES)) == tuple(sizes)
        assert len({w for w, _ in sizes}) == 3 and len({h for _, h in sizes}) == 3
    # a permutation of the sizes must change what the solver does, or solving it proves nothing about which size went where
    a = _candidates(ses.mixed)
    b = _candidates(functools.partial(ses.mixed, ses.MIXED_SIZES_PERMUTED))
    assert any(not np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("l", [1, 2])
def test_level_scene_intensities_use_the_lowest_mantissa_bit(l):
    """the tiled intensity plane keeps the mask in the lowest mantissa bit of I: only intensities that have that bit set can show it"""
    scene = ses.level(l)
    assert scene.level == l and scene.size(0) == (ses.LEVEL_SIZE[0] >> l, ses.LEVEL_SIZE[1] >> l)
    assert np.allclose(scene.intrinsics * (1 << l), scene.window.scene.intrinsics)
    for f in scene.window.frames:
        bits = np.ascontiguousarray(f.pixelinfo[..., 0]).view(np.uint64)
        assert (bits & np.uint64(1)).mean() >= 0.25
