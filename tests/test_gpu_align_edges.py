"""The pose aligner (dsopp_amd/csrc/align.hip) where the parity tests of test_gpu_tracker.py do not reach: explicit non-integer reference
points (push_reference_points and the bilinear reference sample), every validity decision from both sides, a Huber split, the point
counts at which the kernels change their work distribution or their reduction path, and the float32 instantiations.  Checked against
the CPU oracle (full solves) and against the plain model of one linearisation (tests/align_model.py: max_iterations = 1 reports the
initial state's system and the state after one accepted or rejected step).

Bars.  float64: those of test_alignment_parity (iterations and n_valid equal; 1e-8 on energy, pose and H; 1e-6 on the covariance) and of
test_alignment_photometric_parameters (1e-7 on the affine parameters), H
also in the Jacobi-scaled measure align_model.scaled_rel — relative to max |H| the affine prior of 1e12 hides the pose block.
float32: align_model.F32_FACTOR (8) x what single precision does to the same case on the CPU (float32 model against float64 model;
oracle on float32-rounded inputs), computed by the functions tests/test_align_model.py prints the values of — never a device result."""
import numpy as np
import pytest

from dsopp_amd import synthetic as syn

import align_model as am

pytestmark = pytest.mark.gpu


class _Device:
    """pyramids of the cases' images, built once per (image, dtype, mask)"""

    def __init__(self):
        self.pyramids = {}

    def pyramid(self, image, dtype, mask=None):
        from dsopp_amd import capi
        key = (id(image), dtype, None if mask is None else id(mask))
        if key not in self.pyramids:
            H, W = image.shape
            p = capi.Pyramid(W, H, 1, dtype=dtype)
            p.build(image)
            if mask is not None:
                p.set_mask(0, mask)
            self.pyramids[key] = (p, image, mask)   # (the arrays are kept alive: the key is their identity)
        return self.pyramids[key][0]

    def solve(self, c, lm_path=0, dtype=None, **options):
        from dsopp_amd import capi
        dtype = capi.F64 if dtype is None else dtype
        a = capi.HipAligner(capi.default_align_options(dtype=dtype, **am.options_kw(c, **options)))
        try:
            a.set_lm_path(lm_path)
            a.push_reference_points(1000, syn.mat_to_params(c["T_w_ref"]), self.pyramid(c["image_ref"], dtype), 0, c["intr"], c["u"], c["v"], c["idepth"],
                                    c["e_ref"], c["ab_ref"])
            assert a.num_points() == len(c["u"])
            a.push_target(2000, syn.mat_to_params(c["T_w_tgt"]), self.pyramid(c["image_tgt"], dtype, c["mask"]), 0, c["tgt_intr"], c["e_tgt"], c["ab_tgt"])
            return a.solve()
        except capi.HipError as e:
            if not str(e).startswith("dsopp_hip error -1:"):      # anything but a refused argument: the device is in an unknown state,
                pytest.exit(f"device error, nothing more is run: {e}", returncode=3)   # so no further kernel is started in this session
            raise
        finally:
            a.close()

    def close(self):
        for p, _, _ in self.pyramids.values():
            p.close()


@pytest.fixture(scope="module")
def dev():
    d = _Device()
    yield d
    d.close()


def _paths(n):
    return (0, 1) if n <= 1024 else (1,)   # up to 1024 points lm_path 0 is the single-workgroup loop kernel; above only the iteration kernel exists


def _assert_oracle_parity(rg, ro, what):
    print(f"{what}: iterations {rg['iterations']} / {ro['iterations']}, n_valid {rg['n_valid']} / {ro['n_valid']}, energy {abs(rg['energy'] - ro['energy']) / abs(ro['energy']):.2e}, "
          f"pose {np.abs(rg['T_w_target'] - ro['T_w_target']).max():.2e}, H {am.rel(rg['H'], ro['H']):.2e} (scaled {am.scaled_rel(rg['H'], ro['H']):.2e}), "
          f"covariance {am.rel(rg['covariance'], ro['covariance']):.2e}")
    assert rg["iterations"] == ro["iterations"], what
    assert rg["n_valid"] == ro["n_valid"], what
    assert abs(rg["energy"] - ro["energy"]) <= 1e-8 * abs(ro["energy"]), what
    assert abs(rg["rmse"] - ro["rmse"]) <= 1e-8 * ro["rmse"], what
    assert np.abs(rg["T_w_target"] - ro["T_w_target"]).max() <= 1e-8, what
    assert np.abs(rg["affine_brightness"] - ro["affine_brightness"]).max() <= 1e-7, what     # (test_alignment_photometric_parameters' bar)
    assert am.rel(rg["H"], ro["H"]) <= 1e-8 and am.scaled_rel(rg["H"], ro["H"]) <= 1e-8, what
    assert am.rel(rg["covariance"], ro["covariance"]) <= 1e-6, what


def _assert_model_parity(rg, fi, what, bar=None):
    """the device's max_iterations = 1 result against the model's first iteration; bar: dict(H, H_scaled, energy, pose, affine), default 1e-8 (affine 1e-7)"""
    bar = bar or dict(H=1e-8, H_scaled=1e-8, energy=1e-8, pose=1e-8, affine=1e-7)
    T = syn.mat_to_params(fi["T_w_target"])
    got = dict(H=am.rel(rg["H"], fi["H"]), H_scaled=am.scaled_rel(rg["H"], fi["H"]), energy=abs(rg["energy"] - fi["energy"]) / abs(fi["energy"]),
               pose=float(np.abs(rg["T_w_target"] - T).max()), affine=float(np.abs(rg["affine_brightness"] - fi["affine"]).max()))
    got = {k: got[k] for k in bar}
    print(f"{what}: n_valid {rg['n_valid']} / {fi['n_valid']}, accepted {fi['accepted']}; " + ", ".join(f"{k} {got[k]:.2e} (bar {bar[k]:.2e})" for k in got))
    assert rg["iterations"] == 1 and rg["n_valid"] == fi["n_valid"], what
    for k in got:
        assert got[k] <= bar[k], (what, k, got[k], bar[k])


def _both(dev, c, what, paths=None):
    """full solve against the oracle, first iteration against the model, on every LM path the point count has"""
    ro = am.oracle_solve(c)
    fi = am.first_iteration(c)
    for path in paths or _paths(len(c["u"])):
        _assert_oracle_parity(dev.solve(c, path), ro, f"{what} lm_path {path}")
        _assert_model_parity(dev.solve(c, path, max_iterations=1), fi, f"{what} lm_path {path}, one iteration")
    return ro, fi


# ---- 1. explicit points ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["default", "photometric", "weak_prior", "mask", "cameras"])
def test_explicit_points_parity(dev, name):
    """~1500 random non-integer reference positions: the bilinear weights of the reference sample are all non-trivial"""
    c = am.case(name)
    _both(dev, c, name)
    c = am.case(name, 900)       # the single-workgroup loop kernel (lm_path 0 at <= 1024 points)
    _both(dev, c, f"{name} 900")


def test_reference_sample_equals_the_model(dev):
    """the device's reference intensities, seen through the residuals: with a target identical to the reference at the identity pose every
    residual is I_ref(u, v) sampled twice, so the energy vanishes; with the reference intensities of the ORACLE taken from the model's sample
    the parity tests above cover the sample's value (a swapped dx / dy changes every intensity)"""
    c = dict(am.case("default"))
    c.update(image_tgt=c["image_ref"], tgt_planes=c["ref_planes"], T_w_tgt=c["T_w_ref"].copy())
    for path in (0, 1):
        r = dev.solve(c, path, max_iterations=0)
        assert r["n_valid"] == len(c["u"]) and r["iterations"] == 0
        assert r["energy"] <= 1e-20 * len(c["u"]), r["energy"]     # residuals of ~1e-13: the two samples differ by the projection's rounding only


def test_reject_branch(dev):
    c = am.reject_case()
    fi = am.first_iteration(c)
    assert not fi["accepted"]
    for path in (0, 1):
        _assert_model_parity(dev.solve(c, path, max_iterations=1, initial_trust_region_radius=1.0 / c["lambda0"]), fi, f"reject lm_path {path}")


# ---- 2. validity edges -------------------------------------------------------------------------------------------------------------------
def test_validity_edges(dev):
    c = am.edge_case()
    ro, fi = _both(dev, c, "edges")
    assert 0 < ro["n_valid"] < len(c["u"]) / 2


def test_non_finite_reference_points_are_refused(dev):
    from dsopp_amd import capi
    c = am.case("default", 900)
    for k, bad in (("u", np.nan), ("v", np.inf), ("idepth", -np.inf), ("idepth", np.nan), ("u", 1e300)):
        cb = dict(c)
        cb[k] = c[k].copy()
        cb[k][17] = bad
        with pytest.raises(capi.HipError):
            dev.solve(cb)
    _assert_oracle_parity(dev.solve(c), am.oracle_solve(c), "after the refusals")   # nothing was left behind


# ---- 3. Huber split ----------------------------------------------------------------------------------------------------------------------
def test_huber_split(dev):
    c = am.case("huber")
    ro, fi = _both(dev, c, "huber")
    _both(dev, am.case("huber", 900), "huber 900")
    assert 0.3 <= fi["lin0"]["linear"].sum() / fi["n0"] <= 0.7


# ---- 4. point counts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [n for n in am.COUNTS if n > 2])
def test_point_counts(dev, n):
    """255 / 256 / 257: the workgroup edge of the iteration kernel; 511 / 512 / 513: one or two points per lane of the loop kernel; 1024 /
    1025: the switch between the kernels; 10240 / 10241: 40 / 41 workgroups — the partial sums beyond the first 40 go through the tail loop of
    the prologue's reduction; 65536 / 65537 / 70001: the grid is capped at 256 workgroups and a thread sweeps more than one point"""
    c = am.count_case(n)
    _both(dev, c, f"n = {n}")


@pytest.mark.parametrize("n", [1, 2])
def test_rank_deficient_point_counts(dev, n):
    """one or two residuals leave the 8 x 8 system rank deficient: the step is whatever the zero-pivot rule of the solve makes of it.  What is
    defined: the initial state's energy and n_valid, the iteration count, and the state after one iteration where the oracle's step is finite"""
    c = am.count_case(n)
    fi = am.first_iteration(c)
    r0 = am.oracle_solve(c, max_iterations=0)
    ro = am.oracle_solve(c, max_iterations=1)
    rf = am.oracle_solve(c)
    for path in (0, 1):
        g0 = dev.solve(c, path, max_iterations=0)
        assert g0["n_valid"] == r0["n_valid"] == fi["n0"] == n and g0["iterations"] == 0
        assert abs(g0["energy"] - fi["energy0"]) <= 1e-8 * fi["energy0"]
        g1 = dev.solve(c, path, max_iterations=1)
        print(f"n = {n} lm_path {path}: one iteration energy {g1['energy']!r} oracle {ro['energy']!r}, n_valid {g1['n_valid']} / {ro['n_valid']}, "
              f"pose difference {np.abs(g1['T_w_target'] - ro['T_w_target']).max():.2e}; full solve iterations {dev.solve(c, path)['iterations']} / {rf['iterations']}")
        assert g1["iterations"] == ro["iterations"] == 1 and g1["n_valid"] == ro["n_valid"]
        assert abs(g1["energy"] - ro["energy"]) <= 1e-8 * abs(ro["energy"])
        if np.all(np.isfinite(ro["T_w_target"])) and np.all(np.isfinite(ro["H"])):
            assert np.abs(g1["T_w_target"] - ro["T_w_target"]).max() <= 1e-8
        assert dev.solve(c, path)["iterations"] == rf["iterations"]


def test_no_points(dev):
    c = dict(am.case("default"))
    for k in ("u", "v", "idepth", "intensity"):
        c[k] = np.zeros(0)
    for path in (0, 1):
        r = dev.solve(c, path)
        assert r["n_valid"] == 0 and r["iterations"] == 0


# ---- 5. float32 --------------------------------------------------------------------------------------------------------------------------
def _f32_bar(name, n):
    s = am.f32_first_iteration_sensitivity(name, n)
    return {k: am.F32_FACTOR * s[k] for k in ("H", "H_scaled", "energy", "pose")}   # (the affine parameters barely move under the 1e12 prior)


@pytest.mark.parametrize("name,n", [("default", 1500), ("photometric", 1500), ("default", 900), ("photometric", 900)])
def test_float32_first_iteration(dev, name, n):
    """5a: the float32 sweep (casts of M, U, points and intensities, float reciprocal, float texels) against the float64 model"""
    from dsopp_amd import capi
    c = am.case(name, n, True)
    fi = am.first_iteration(c)
    for path in _paths(n):
        _assert_model_parity(dev.solve(c, path, dtype=capi.F32, max_iterations=1), fi, f"float32 {name} {n} lm_path {path}", _f32_bar(name, n))


@pytest.mark.parametrize("n", [900, 1500])
def test_float32_full_solve(dev, n):
    """5b: both LM paths on float32 inputs: the same iterations and n_valid, the pose to 1e-6 (the sweep is the same code, the two reductions
    add in different orders); the end pose within 8 x the oracle's own sensitivity to float32-rounded inputs of the float64 oracle.  The
    case (exposures and affine of both frames) takes no termination decision near its threshold — guarded on the CPU, where the float32
    model run through the whole loop ends 4.8e-7 (n = 1500) and 5.5e-7 (n = 900) off the float64 run, inside the bars of 9.8e-7 and 1.6e-6."""
    from dsopp_amd import capi
    c = am.case("photometric", n, True)
    ro = am.oracle_solve(c)
    s = am.f32_end_state_sensitivity("photometric", n)
    r0, r1 = dev.solve(c, 0, dtype=capi.F32), dev.solve(c, 1, dtype=capi.F32)
    print(f"float32 full solve n = {n}: iterations {r0['iterations']} / {r1['iterations']} (oracle {ro['iterations']}), n_valid {r0['n_valid']} / {r1['n_valid']} "
          f"(oracle {ro['n_valid']}), paths differ by {np.abs(r0['T_w_target'] - r1['T_w_target']).max():.2e}, end pose off the oracle by "
          f"{np.abs(r0['T_w_target'] - ro['T_w_target']).max():.2e} / {np.abs(r1['T_w_target'] - ro['T_w_target']).max():.2e} (bar {am.F32_FACTOR * s['pose']:.2e}), "
          f"affine {np.abs(r1['affine_brightness'] - ro['affine_brightness']).max():.2e}")
    assert r0["iterations"] == r1["iterations"] and r0["n_valid"] == r1["n_valid"]
    assert np.abs(r0["T_w_target"] - r1["T_w_target"]).max() <= 1e-6
    for r in (r0, r1):
        assert np.abs(r["T_w_target"] - ro["T_w_target"]).max() <= am.F32_FACTOR * s["pose"]


def test_float32_estimate_pose_persistent_equals_launch_per_iteration():
    """5c: test_estimate_pose_persistent_launch_equals_launch_per_iteration (tests/test_depth_maps.py) with float32 pyramids and a float32
    aligner, 3 levels at 320 x 240, a hopeless hypothesis in front of the good one"""
    from dsopp_amd import capi
    W, H, L = 320, 240, 3
    win = syn.make_window(num_frames=4, num_points=1200, width=W, height=H, seed=29)
    g = syn.load_window(capi.HipWindow(capi.default_pba_options()), win)
    g.solve()
    maps = g.create_reference_depth_maps(L)
    newest, target = win.frames[-1], win.frames[-2]
    pr, pt = capi.Pyramid(W, H, L, dtype=capi.F32), capi.Pyramid(W, H, L, dtype=capi.F32)
    pr.build(newest.image_u8)
    pt.build(target.image_u8)
    T_ref, ab_ref = g.get_pose(newest.frame_id)
    T_good = syn.mat_to_params(target.T_w_c_init)
    T_bad = syn.mat_to_params(target.T_w_c_gt @ syn.se3_exp(np.array([1.5, -1.0, 0.8, 0.3, -0.4, 0.25])))
    out = []
    for path in (0, 1):
        a = capi.HipAligner(capi.default_align_options(dtype=capi.F32))
        a.set_lm_path(path)
        rmse_last = np.full(L, 1e10)
        f0 = a.estimate_pose(newest.timestamp, T_ref, pr, maps, 1.0, ab_ref, newest.timestamp + 1, pt, 1.0, win.scene.intrinsics, T_good[None, :], np.zeros(2), rmse_last)
        r0 = rmse_last.copy()
        f1 = a.estimate_pose(newest.timestamp, T_ref, pr, maps, 1.0, ab_ref, newest.timestamp + 2, pt, 1.0, win.scene.intrinsics, np.stack([T_bad, T_good]), np.zeros(2),
                             rmse_last)
        out.append((f0, r0, f1, rmse_last.copy()))
        a.close()
    (f0, r0, f1, r1), (h0, s0, h1, s1) = out
    print(f"float32 estimate_pose: iterations {f0['lm_iterations']} / {h0['lm_iterations']} and {f1['lm_iterations']} / {h1['lm_iterations']}, tries {f1['tries']} / {h1['tries']}, "
          f"rmse {r0} / {s0} and {r1} / {s1}, pose difference {np.abs(f1['T_w_target'] - h1['T_w_target']).max():.2e}")
    assert f0["success"] and h0["success"] and f0["tries"] == h0["tries"] == 1
    assert f1["success"] and h1["success"] and f1["tries"] == h1["tries"] == 2, (f1["tries"], h1["tries"])
    for fa, fb in ((f0, h0), (f1, h1)):
        assert fa["lm_iterations"] == fb["lm_iterations"], (fa["lm_iterations"], fb["lm_iterations"])
    assert np.allclose(r0, s0, rtol=1e-12) and np.allclose(r1, s1, rtol=1e-12)
    for obj in (maps, pr, pt, g):
        obj.close()


def test_float32_reference_sample(dev):
    """5d: sampleReferenceKernel<float> through push_reference_points: a target identical to the reference at the identity pose leaves
    residuals of float32 round-off only.  The projection of the identity is exact in float32 here, so the float32 model's residuals
    vanish identically and give no bar; the bar is the round-off of the two bilinear blends instead: four products of a weight <= 1
    with an intensity <= 255, each and their sums rounded to 2^-24 relative, |error| <= 8 x 255 x 2^-24 = 1.2e-4 per residual at the
    very most (compilers may contract the two blends differently), so energy <= n (1.2e-4)^2 / 2.  A wrong stride, lane or weight
    leaves residuals of grey levels: energy ~ 10 n."""
    from dsopp_amd import capi
    c = dict(am.case("default", 1500, True))
    c.update(image_tgt=c["image_ref"], tgt_planes=c["ref_planes"], T_w_tgt=c["T_w_ref"].copy())
    n = len(c["u"])
    e32 = am.first_iteration(c, dtype=np.float32, intensity=am.reference_intensity(c["ref_planes"], c["u"], c["v"], np.float32))["energy0"]
    bar = n * (8 * 255 * 2.0 ** -24) ** 2 / 2
    assert e32 <= bar
    for path in (0, 1):
        r = dev.solve(c, path, dtype=capi.F32, max_iterations=0)
        print(f"float32 reference sample lm_path {path}: energy {r['energy']:.3e} (float32 model {e32:.3e}, bar {bar:.3e}), n_valid {r['n_valid']}")
        assert r["n_valid"] == n and r["iterations"] == 0
        assert r["energy"] <= bar
        assert dev.solve(c, path, dtype=capi.F32)["energy"] <= bar
