"""tests/point_cloud_model.py, the NumPy statement of the map's update and export rules (include/dsopp_hip.h, "the map"), on hand-worked
cases: every branch of the update rule, the class predicate and the strict filters at equality, the exporter's skip, the world transform
against synthetic.params_to_mat, and the colour tables.  tests/test_gpu_point_cloud.py holds the device to the model exactly."""
import numpy as np
import pytest

import point_cloud_model as pc
from dsopp_amd import synthetic as syn

K = np.array([300.0, 310.0, 32.0, 24.0])
IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.float64)


def fresh():
    return pc.Keyframe(7, K.copy(), IDENTITY.copy())


def update(kf, idepth, inv_hdd=None, baseline=None, flags=None, uv=None, **kw):
    n = len(idepth)
    return pc.update_keyframe(kf, np.zeros((n, 2)) + 5.0 if uv is None else uv, np.asarray(idepth, dtype=np.float64),
                              np.full(n, 1e-6) if inv_hdd is None else inv_hdd, np.full(n, 0.2) if baseline is None else baseline,
                              np.zeros(n, dtype=np.uint8) if flags is None else np.asarray(flags, dtype=np.uint8), **kw)


def test_new_record_and_the_idepth_branches():
    below, above = np.nextafter(1e-8, 0.0), 1e-8
    kf = update(fresh(), [0.5, below, -below, above, -above, -0.25])
    assert kf.n == 6
    # |idepth| < 1e-8 on either side: 0; at 1e-8: kept; negative: an outlier whose record keeps the idepth it was created with
    assert kf.idepth.tolist() == [0.5, 0.0, 0.0, above, -above, -0.25]
    assert kf.flags.tolist() == [0, 0, 0, 0, pc.FLAG_OUTLIER, pc.FLAG_OUTLIER]
    assert np.all(kf.variance == 1e-6) and np.all(kf.relative_baseline == 0.2)
    assert np.all(kf.type == 0) and np.all(kf.rgb == 0) and np.all(kf.uv == 5.0)


def test_variance_takes_the_channels_or_the_constant():
    kf = update(fresh(), [0.5, 0.5], inv_hdd=np.array([3e-7, 0.1]), channels=3)
    assert kf.variance.tolist() == [np.float64(3e-7) * 3.0, np.float64(0.1) * 3.0]
    kf = update(fresh(), [0.5, 0.5], inv_hdd=np.array([3e-7, 0.1]), estimate_uncertainty=False)
    assert kf.variance.tolist() == [1e-5, 1e-5]


def test_outlier_is_sticky_and_the_baseline_is_a_running_maximum():
    kf = update(fresh(), [0.5, 0.5], baseline=np.array([0.3, 0.1]), flags=[pc.WINDOW_OUTLIER, 0])
    assert kf.flags.tolist() == [pc.FLAG_OUTLIER, 0]
    kf = update(kf, [0.6, 0.6], baseline=np.array([0.2, 0.4]), flags=[0, 0])   # the window's flag is gone: the record's stays
    assert kf.flags.tolist() == [pc.FLAG_OUTLIER, 0]
    assert kf.relative_baseline.tolist() == [0.3, 0.4] and kf.idepth.tolist() == [0.6, 0.6]
    kf = update(kf, [0.6, 0.6], baseline=np.array([0.25, 0.35]))
    assert kf.relative_baseline.tolist() == [0.3, 0.4]


def test_marginalize_at_the_bound_and_one_ulp_above():
    """variance / idepth > 1e-3 is strict: idepth = 1, so the quotient is the variance itself"""
    at, above = 1e-3, np.nextafter(1e-3, 1.0)
    kf = update(fresh(), [1.0, 1.0, 1.0], inv_hdd=np.array([at, above, 1e-9]))
    kf = update(kf, [1.0, 1.0, 1.0], inv_hdd=np.zeros(3), flags=[pc.WINDOW_MARGINALIZED] * 3)
    assert kf.flags.tolist() == [pc.FLAG_MARGINALIZED, pc.FLAG_MARGINALIZED | pc.FLAG_OUTLIER, pc.FLAG_MARGINALIZED]
    assert kf.variance.tolist() == [at, above, 1e-9]   # rule 3 did not run: the window's inv_hdd = 0 was not taken


def test_marginalize_negative_zero_and_never_updated():
    kf = update(fresh(), [-0.5, 0.0, 0.5])   # the first is an outlier already; the second has idepth 0
    kf2 = update(kf.copy(), [-0.5, 0.0, 0.5], flags=[pc.WINDOW_MARGINALIZED] * 3)
    assert kf2.flags.tolist() == [pc.FLAG_MARGINALIZED | pc.FLAG_OUTLIER, pc.FLAG_MARGINALIZED | pc.FLAG_OUTLIER, pc.FLAG_MARGINALIZED]
    # (1e-6 / 0 = inf > 1e-3: an outlier, as in the reference)
    # a landmark first seen already marginalised keeps variance DBL_MAX: an outlier
    first = update(fresh(), [0.5], flags=[pc.WINDOW_MARGINALIZED])
    assert first.variance[0] == pc.DBL_MAX and first.flags[0] == pc.FLAG_MARGINALIZED | pc.FLAG_OUTLIER and first.relative_baseline[0] == 0.0


def test_marginalised_record_is_frozen():
    kf = update(fresh(), [0.5], inv_hdd=np.array([1e-7]), baseline=np.array([0.3]))
    kf = update(kf, [0.9], inv_hdd=np.array([5.0]), baseline=np.array([0.9]), flags=[pc.WINDOW_MARGINALIZED])
    assert (kf.idepth[0], kf.variance[0], kf.relative_baseline[0], kf.flags[0]) == (0.5, 1e-7, 0.3, pc.FLAG_MARGINALIZED)
    kf = update(kf, [-3.0], inv_hdd=np.array([7.0]), baseline=np.array([2.0]), flags=[pc.WINDOW_MARGINALIZED])
    assert (kf.idepth[0], kf.variance[0], kf.relative_baseline[0], kf.flags[0]) == (0.5, 1e-7, 0.3, pc.FLAG_MARGINALIZED)
    # an outlier flag of the window still reaches it
    kf = update(kf, [-3.0], flags=[pc.WINDOW_MARGINALIZED | pc.WINDOW_OUTLIER])
    assert kf.flags[0] == pc.FLAG_MARGINALIZED | pc.FLAG_OUTLIER and kf.idepth[0] == 0.5


def test_appended_landmarks_and_image_colours():
    bgr = np.arange(4 * 6 * 3, dtype=np.uint8).reshape(4, 6, 3)
    uv = np.array([[2.9, 1.2], [5.99, 3.99], [6.0, 1.0], [-0.5, 1.0], [1.0, 4.0]])
    kf = update(fresh(), np.full(5, 0.5), uv=uv, image=bgr)
    assert kf.rgb.tolist() == [bgr[1, 2, ::-1].tolist(), bgr[3, 5, ::-1].tolist(), [0, 0, 0], [0, 0, 0], [0, 0, 0]]
    grey = bgr[:, :, 0]
    more = np.vstack([uv, [[0.0, 0.0]]])
    kf = update(kf, np.full(6, 0.5), uv=more + 1.0, image=grey)   # the old records keep uv and colour; the new one is sampled
    assert np.array_equal(kf.uv[:5], uv) and kf.uv[5].tolist() == [1.0, 1.0]
    assert kf.rgb[5].tolist() == [int(grey[1, 1])] * 3 and kf.rgb[0].tolist() == bgr[1, 2, ::-1].tolist()


def test_semantic_type():
    hist = np.zeros((3, 256), dtype=np.uint8)
    hist[0, [4, 9]] = 3, 3          # a tie: the first
    hist[1, [4, 200]] = 5, 2
    weights = np.zeros(256, dtype=np.uint64)
    weights[200] = 10
    kf = update(fresh(), np.full(3, 0.5), hist=hist)
    assert kf.type.tolist() == [4, 4, 0]
    kf = update(kf, np.full(3, 0.5), hist=hist, weights=weights)
    assert kf.type.tolist() == [4, 200, 0]   # all weights times counts zero: the plain maximum
    kf = update(kf, np.full(3, 0.5))         # no observations: the types stay
    assert kf.type.tolist() == [4, 200, 0]


def records(idepth, variance, baseline, flags, pose=IDENTITY, type=None, rgb=None, uv=None):
    n = len(idepth)
    return pc.keyframe_from_records(0, K, pose, np.zeros((n, 2)) + 40.0 if uv is None else uv, idepth, variance, baseline, flags, type, rgb)


def test_class_predicate_and_its_edges():
    M, O = pc.FLAG_MARGINALIZED, pc.FLAG_OUTLIER
    kf = records([0.5] * 4 + [0.0, 0.5, 0.5], [1e-9] * 7, [0.2] * 5 + [0.1, np.nextafter(0.1, 1.0)], [0, M, O, M | O, 0, 0, 0])
    got = {c: pc.export([kf], classes=c)["record_index"].tolist() for c in (1, 2, 4, 3, 7, 0)}
    # idepth == 0 and relative_baseline == 0.1 never pass; an outlier goes to the outlier class only, marginalised or not
    assert got == {1: [0, 6], 2: [1], 4: [2, 3], 3: [0, 1, 6], 7: [0, 1, 2, 3, 6], 0: []}


def test_filters_are_strict():
    var, rb = 5e-8, 0.15
    kf = records([0.5] * 4, [var, np.nextafter(var, 0.0), 1e-9, 1e-9], [0.2, 0.2, rb, np.nextafter(rb, 1.0)], [0] * 4)
    assert pc.export([kf], apply_filters=True)["record_index"].tolist() == [1, 3]
    assert pc.export([kf], apply_filters=False)["record_index"].tolist() == [0, 1, 2, 3]
    assert pc.export([kf], apply_filters=True, max_idepth_variance=1.0, min_relative_baseline_filter=0.0)["record_index"].tolist() == [0, 1, 2, 3]


def test_world_frame_skips_tiny_idepth():
    tiny, at = np.nextafter(1e-16, 0.0), 1e-16
    kf = records([tiny, at, -tiny], [1e-9] * 3, [0.2] * 3, [0] * 3)
    assert pc.export([kf], frame=pc.FRAME_WORLD)["record_index"].tolist() == [1]
    assert pc.export([kf], frame=pc.FRAME_KEYFRAME)["record_index"].tolist() == [0, 1, 2]


def test_keyframe_frame_is_the_pinhole_ray_over_idepth():
    kf = records([0.25], [1e-9], [0.2], [0], uv=np.array([[62.0, 55.0]]))
    xyz = pc.export([kf], frame=pc.FRAME_KEYFRAME)["xyz"][0]
    ifx, ify = 1.0 / 300.0, 1.0 / 310.0
    assert xyz.tolist() == [(62.0 - 32.0) * ifx / 0.25, (55.0 - 24.0) * ify / 0.25, 4.0]


def test_world_transform_against_params_to_mat():
    """x = T [d, idepth], x[:3] / x[3] with T from synthetic.params_to_mat: the model's own order of operations differs from the matrix
    product's only by rounding — a handful of products and sums of terms no larger than |R d| + |t| idepth, so the two agree within a
    few ulps of (1 + |X|); 1e-12 is far above that and far below any error of the formula"""
    rng = np.random.default_rng(5)
    for _ in range(20):
        q = rng.normal(size=4)
        pose = np.concatenate([q / np.linalg.norm(q), rng.normal(size=3) * 10])
        n = 16
        uv = rng.uniform(0, 64, size=(n, 2))
        idepth = rng.uniform(0.05, 2.0, size=n)
        kf = records(idepth, [1e-9] * n, [0.2] * n, [0] * n, pose=pose, uv=uv)
        got = pc.export([kf])["xyz"]
        T = syn.params_to_mat(pose)
        for i in range(n):
            d = np.array([(uv[i, 0] - K[2]) / K[0], (uv[i, 1] - K[3]) / K[1], 1.0, idepth[i]])
            x = T @ d
            X = x[:3] / x[3]
            assert np.all(np.abs(got[i] - X) <= 1e-12 * (1 + np.abs(X))), (got[i], X)


def test_colour_tables():
    M, O = pc.FLAG_MARGINALIZED, pc.FLAG_OUTLIER
    rgb = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12]], dtype=np.uint8)
    kf = records([0.5] * 4, [1e-9] * 4, [0.2] * 4, [0, M, O, M | O], type=[0, 13, 14, 255], rgb=rgb)
    ex = lambda scheme: pc.export([kf], classes=pc.CLASS_ALL, colours=scheme)["rgb"].tolist()
    assert ex(pc.COLOURS_LANDMARK_TYPE) == [[100, 255, 100], [255, 100, 100], [255, 0, 0], [255, 0, 0]]
    assert ex(pc.COLOURS_CONSTANT) == [[200, 200, 200]] * 4
    assert ex(pc.COLOURS_SEMANTIC) == [[200, 200, 200], [139, 0, 255], [200, 200, 200], [255, 255, 153]]   # 14 % 14 = 0, 255 % 14 = 3
    assert ex(pc.COLOURS_IMAGE) == rgb.tolist()
    assert pc.SEMANTIC_COLOURS.shape == (14, 3) and pc.SEMANTIC_COLOURS[3].tolist() == [255, 255, 153]
    without = records([0.5], [1e-9], [0.2], [0])
    with pytest.raises(pc.StateError):
        pc.export([kf, without], colours=pc.COLOURS_IMAGE)


def test_canonical_order_and_counts():
    a = records([0.5, 0.0, 0.5], [1e-9] * 3, [0.2] * 3, [0] * 3)
    empty = records([], [], [], [])
    b = records([0.5, 0.5], [1e-9] * 2, [0.2, 0.05], [0] * 2)
    out = pc.export([empty, a, empty, b, empty])
    assert out["count"] == 3 and out["per_keyframe_counts"].tolist() == [0, 2, 0, 1, 0]
    assert out["keyframe_index"].tolist() == [1, 1, 3] and out["record_index"].tolist() == [0, 2, 0]
    assert out["type"].dtype == np.uint8 and out["xyz"].shape == (3, 3)
    assert pc.export([])["count"] == 0 and pc.export([])["xyz"].shape == (0, 3)


def build_example(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "dsopp_amd", "lib")
    exe = str(tmp_path / "example_point_cloud")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", os.path.join(root, "dsopp_amd", "host", "example_point_cloud.cpp"),
                           f"-L{libdir}", "-ldsopp_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", exe])
    return exe


def test_example_driver_compiles_and_fails_loudly_without_gpu(tmp_path):
    import subprocess
    from dsopp_amd import capi
    exe = build_example(tmp_path)
    if capi.device_count() > 0:
        pytest.skip("GPU present: tests/test_gpu_point_cloud.py runs it")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "no CPU fallback" in r.stdout
