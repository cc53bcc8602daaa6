"""The plain model of one aligner linearisation (tests/align_model.py) against the CPU oracle and against finite differences, the guards
of the case generators the device tests use (tests/test_gpu_align_edges.py), and the measurement of what single precision does to a
case — the source of the float32 bars of the device tests.  Nothing here needs a GPU."""
import numpy as np
import pytest

from dsopp_amd import synthetic as syn

import align_model as am

PARITY_CASES = ("default", "photometric", "weak_prior", "mask", "huber", "cameras", "edges")
F32_CASES = (("default", 1500), ("photometric", 1500), ("default", 900), ("photometric", 900))   # first iteration in float32 on the device
F32_FULL_CASES = (("photometric", 900), ("photometric", 1500))                                       # full float32 solves on the device


def _get(name):
    return am.edge_case() if name == "edges" else am.case(name)


def test_case_constants_are_the_library_defaults():
    from oracle import pyoracle as po
    o = po.default_align_options()
    assert o.sigma_huber_loss == am.DEFAULT_SIGMA and tuple(o.affine_brightness_regularizer) == am.DEFAULT_REG
    assert 1.0 / o.initial_trust_region_radius == am.case("default")["lambda0"]
    assert (o.max_iterations, o.function_tolerance, o.parameter_tolerance) == (50, 1e-5, 1e-5)          # lm_solve's defaults
    # the planes of the cases are level 0 of the pyramid both solvers build from the 8-bit image
    win, pr, pt = am.frames()
    for f, planes in zip(win.frames, (pr, pt)):
        infos, _ = po.build_pyramid(f.image_u8, levels=1)
        assert np.array_equal(infos[0], planes)
    assert np.array_equal(am.forward_target()[1].astype(np.float32).astype(np.float64), am.forward_target()[1])   # exact in float32


def test_oracle_reports_the_initial_system_after_one_iteration():
    """max_iterations = 1: linearize at the initial state, one step, energy at the candidate, accept or reject, end.  The reported H is the
    system the step was solved from — the INITIAL state's — while energy, n_valid, pose and affine are the candidate's once accepted."""
    c = am.case("photometric")
    fi = am.first_iteration(c)
    ro = am.oracle_solve(c, max_iterations=1)
    assert ro["iterations"] == 1 and fi["accepted"]
    H1 = fi["lin1"]["H"]
    assert am.scaled_rel(ro["H"], fi["H"]) <= 1e-10 < 1e-4 < am.scaled_rel(ro["H"], H1)
    assert abs(ro["energy"] - fi["lin1"]["energy"]) <= 1e-10 * ro["energy"] < 1e-3 * ro["energy"] < abs(ro["energy"] - fi["energy0"])
    r0 = am.oracle_solve(c, max_iterations=0)
    assert r0["iterations"] == 0 and abs(r0["energy"] - fi["energy0"]) <= 1e-10 * fi["energy0"] and r0["n_valid"] == fi["n0"]


@pytest.mark.parametrize("name", PARITY_CASES)
def test_model_equals_oracle_on_the_first_linearisation(name):
    c = _get(name)
    fi = am.first_iteration(c)
    ro = am.oracle_solve(c, max_iterations=1)
    assert ro["iterations"] == 1
    assert fi["n_valid"] == ro["n_valid"] and 0 < ro["n_valid"] < len(c["u"])
    assert am.rel(fi["H"], ro["H"]) <= 1e-10 and am.scaled_rel(fi["H"], ro["H"]) <= 1e-10
    assert abs(fi["energy"] - ro["energy"]) <= 1e-10 * abs(ro["energy"])
    assert np.abs(syn.mat_to_params(fi["T_w_target"]) - ro["T_w_target"]).max() <= 1e-10
    assert np.abs(fi["affine"] - ro["affine_brightness"]).max() <= 1e-10 * max(1.0, np.abs(ro["affine_brightness"]).max())
    assert np.abs(ro["T_w_target"] - syn.mat_to_params(c["T_w_tgt"])).max() > 1e-5            # the step is not a no-op
    if name == "weak_prior":
        assert np.abs(fi["affine"] - c["ab_tgt"]).max() > 1e-3                                  # the affine columns moved something


def test_model_reject_branch_equals_oracle():
    """a first step that is REJECTED: the target's brightness factor starts at exp(-2) under a weak prior, the undamped Gauss-Newton step
    in a (linear in exp(a)) overshoots to exp(+4.4) and the energy rises a hundredfold.  The reported state is the initial one."""
    c = am.reject_case()
    fi = am.first_iteration(c)
    ro = am.oracle_solve(c, max_iterations=1, initial_trust_region_radius=1.0 / c["lambda0"])
    assert not fi["accepted"] and fi["lin1"] is not None and fi["lin1"]["energy"] > 10 * fi["energy0"]
    assert ro["iterations"] == 1 and ro["n_valid"] == fi["n0"] and abs(ro["energy"] - fi["energy0"]) <= 1e-10 * fi["energy0"]
    assert np.abs(ro["T_w_target"] - syn.mat_to_params(c["T_w_tgt"])).max() <= 1e-12
    assert np.array_equal(ro["affine_brightness"], c["ab_tgt"])
    assert am.scaled_rel(fi["H"], ro["H"]) <= 1e-10


@pytest.mark.parametrize("name", ["default", "photometric", "weak_prior", "mask", "huber", "edges"])
def test_model_lm_loop_equals_oracle_full_solve(name):
    """the accept / reject / converge logic around the linearisation, stated once more: same iteration count, same end state"""
    c = _get(name)
    ro, rm = am.oracle_solve(c), am.lm_solve(c)
    assert rm["iterations"] == ro["iterations"] and rm["n_valid"] == ro["n_valid"] and 2 < ro["iterations"] < 50
    assert abs(rm["energy"] - ro["energy"]) <= 1e-10 * ro["energy"]
    assert np.abs(syn.mat_to_params(rm["T_w_target"]) - ro["T_w_target"]).max() <= 1e-10
    assert np.abs(rm["affine"] - ro["affine_brightness"]).max() <= 1e-10 * max(1.0, np.abs(ro["affine_brightness"]).max())
    assert any(not acc for _, _, acc in rm["trace"]) or name == "default"     # rejected steps occur on the way


def _bilinear_exact_planes(W, H):
    """an image that bilinear interpolation reproduces exactly, I = a x + b y + c x y + d: its central differences are its exact partial
    derivatives, and they are again reproduced exactly by their own bilinear blend"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    a, b, cc, d = 0.9, -0.6, 0.004, 40.0
    planes = np.stack([a * xx + b * yy + cc * xx * yy + d, a + cc * yy, b + cc * xx], axis=2)
    assert np.abs(syn.pixelinfo_from_plane(planes[..., 0])[2:-2, 2:-2] - planes[2:-2, 2:-2]).max() <= 1e-12
    return planes


def _residuals(c, planes, T_tr, cand_ab):
    return am.linearize(c["u"], c["v"], c["idepth"], c["intensity"], planes, None, c["intr"], c["size"], c["tgt_intr"], T_tr, c["e_ref"], c["ab_ref"], c["e_tgt"],
                        c["ab_tgt"], cand_ab, c["sigma"], c["reg"])


@pytest.mark.parametrize("name", ["photometric", "cameras"])
def test_model_jacobian_equals_central_differences(name):
    """The row of the normal equations is (-dr / d eps, +dr / d a, +dr / d b) for the left perturbation exp(eps) T.

    The row blends the STORED gradient planes; that is the derivative of the blended intensity only where the stored gradients are the
    image's own partial derivatives.  On a camera image they are central differences while the blend's slope inside a cell is a forward
    difference, so a finite difference of the residual does not reproduce the row there at any distance from the texel edges.  The check
    therefore runs in two parts: (1) on an image that bilinear interpolation reproduces exactly, where the residual is differentiable
    everywhere (no point has to be skipped) and the finite difference of the WHOLE residual must give the row; (2) on the camera image, the
    geometric factor d (tu, tv) / d eps of the row by finite differences of the model's own projection, and the two affine columns by
    finite differences of the residual (both smooth everywhere, texel edges included)."""
    c = am.case(name)
    W, H = c["size"]
    T0 = np.linalg.inv(c["T_w_tgt"]) @ c["T_w_ref"]
    h = 1e-6
    for planes, whole in ((_bilinear_exact_planes(W, H), True), (c["tgt_planes"], False)):
        l0 = _residuals(c, planes, T0, (0.0, 0.0))
        ok = l0["valid"].copy()
        fd = np.zeros((len(c["u"]), 8))
        for k in range(8):
            lp, lm = (_residuals(c, planes, am.se3_exp(sg * h * np.eye(6)[k]) @ T0 if k < 6 else T0,
                                 (0.0, 0.0) if k < 6 else tuple(sg * h * np.eye(2)[k - 6])) for sg in (1.0, -1.0))
            ok &= lp["valid"] & lm["valid"]
            if whole or k >= 6:
                fd[:, k] = (lp["residual"] - lm["residual"]) / (2 * h)
            else:
                fd[:, k] = (l0["sample"][:, 1] * (lp["tu"] - lm["tu"]) + l0["sample"][:, 2] * (lp["tv"] - lm["tv"])) / (2 * h)
        skipped = 1.0 - ok.sum() / l0["valid"].sum()
        assert skipped < 0.2 and ok.sum() > 1000, skipped          # (only points that leave the ROI under the perturbation)
        want = l0["row"][ok] * np.array([-1.0] * 6 + [1.0, 1.0])
        scale = np.maximum(np.abs(want).max(axis=0), 1.0)
        err = np.abs(fd[ok] - want).max(axis=0) / scale
        # central differences with h = 1e-6: truncation ~ h^2, rounding ~ 255 x 2^-53 / h = 3e-8 of a residual against columns of 1e1 .. 1e3
        assert err.max() <= 1e-6, (whole, err)
        assert np.abs(want).max(axis=0).min() > 0.5                 # no column is trivially zero


# ---------------------------------------------------------------------------------------------------------------------------------------
# guards of the generators
# ---------------------------------------------------------------------------------------------------------------------------------------
def _min_margin(c, lin):
    return am.margins(lin, c["size"], c["size"], c["sigma"], c["u"], c["v"], c["idepth"], c["mask"] is not None).min()


@pytest.mark.parametrize("name", PARITY_CASES)
def test_no_generated_point_sits_on_a_decision_edge(name):
    c = _get(name)
    assert _min_margin(c, am.first_iteration(c)["lin0"]) >= am.F64_MARGIN


@pytest.mark.parametrize("n", am.COUNTS)
def test_no_point_of_a_count_case_sits_on_a_decision_edge(n):
    c = am.count_case(n)
    fi = am.first_iteration(c)
    assert len(c["u"]) == n and fi["n0"] == n                       # drawn from valid positions: n = 1 and 2 have residuals
    assert _min_margin(c, fi["lin0"]) >= am.F64_MARGIN
    assert np.all(c["u"] != np.rint(c["u"])) and np.all(c["v"] != np.rint(c["v"]))


@pytest.mark.parametrize("name,n", F32_CASES)
def test_float32_cases_keep_clear_of_every_decision_edge(name, n):
    """at the initial state and at the first candidate: n_valid of a float32 evaluation is then well defined"""
    c = am.case(name, n, True)
    fi = am.first_iteration(c)
    assert len(c["u"]) == n and fi["lin1"] is not None
    assert _min_margin(c, fi["lin0"]) >= am.F32_MARGIN and _min_margin(c, fi["lin1"]) >= am.F32_MARGIN
    f32 = am.first_iteration(c, dtype=np.float32)
    assert np.array_equal(f32["lin0"]["reason"], fi["lin0"]["reason"]) and np.array_equal(f32["lin1"]["reason"], fi["lin1"]["reason"])
    assert np.array_equal(f32["lin0"]["linear"], fi["lin0"]["linear"])


@pytest.mark.parametrize("name,n", F32_FULL_CASES)
def test_float32_full_solve_cases_take_no_termination_decision_on_its_edge(name, n):
    """|de| / e < function_tolerance and |x|^2 < parameter_tolerance (...) end the loop.  Single precision moves the energy by a few 1e-8
    (this case) to 1e-5 (relative), so a run whose ratios pass 1 slowly ends an iteration earlier or later in float32 and its end pose
    differs by that iteration's step — a property of the termination rule, not of the arithmetic under test.  The cases of the full
    float32 solves are of the kind whose energy single precision moves by less than 1e-6 relative (asserted), i.e. whose ratio
    |de| / e / function_tolerance it moves by less than 0.2, and take every termination decision at least 0.25 away from the threshold 1;
    the float32 model run through the same loop then takes the same number of iterations."""
    c = am.case(name, n, True)
    r64 = am.lm_solve(c)
    for rf, rp, accepted in r64["trace"]:
        assert abs(rf - 1.0) >= 0.25, r64["trace"]
        assert not accepted or abs(rp - 1.0) >= 0.25, r64["trace"]
    assert am.f32_first_iteration_sensitivity(name, n)["energy"] < 1e-6
    r32 = am.lm_solve(c, dtype=np.float32, intensity=am.reference_intensity(c["ref_planes"], c["u"], c["v"], np.float32))
    assert r32["iterations"] == r64["iterations"] == am.oracle_solve(c)["iterations"] and r32["n_valid"] == r64["n_valid"]
    print(f"float32 model through the whole loop, {name} n={n}: end pose off the float64 run by "
          f"{np.abs(syn.mat_to_params(r32['T_w_target']) - syn.mat_to_params(r64['T_w_target'])).max():.3e}")


def test_huber_case_splits_its_residuals():
    c = am.case("huber")
    l0 = am.first_iteration(c)["lin0"]
    frac = l0["linear"].sum() / l0["n_valid"]
    assert c["sigma"] == am.HUBER_SIGMA and 0.3 <= frac <= 0.7, frac
    # and the default case is (nearly) all quadratic: the two cases differ in the branch they exercise
    d0 = am.first_iteration(am.case("default"))["lin0"]
    assert d0["linear"].sum() / d0["n_valid"] < 0.05


def test_edge_case_contains_every_validity_reason():
    c = am.edge_case()
    fi = am.first_iteration(c)
    counts = np.bincount(fi["lin0"]["reason"], minlength=len(am.REASONS))
    assert np.all(counts >= 5), dict(zip(am.REASONS, counts))
    l0, W, H = fi["lin0"], *c["size"]
    reached = (l0["reason"] == 0) | (l0["reason"] >= 4)              # points that got as far as the target ROI test
    tu, tv = l0["tu"][reached], l0["tv"][reached]
    for lo, hi, t in ((am.BORDER, W - am.BORDER - 1, tu), (am.BORDER, H - am.BORDER - 1, tv)):
        for edge, sign in ((lo, 1.0), (hi, -1.0)):
            d = sign * (t - edge)
            assert ((d > 0) & (d < 0.5)).sum() >= 5 and ((d < 0) & (d > -0.5)).sum() >= 5   # both sides of every target bound
    # both sides of .5 in x and in y, with both outcomes of the mask lookup
    m = (l0["reason"] == 0) | (l0["reason"] == 5)
    for t in (l0["tu"][m], l0["tv"][m]):
        f = t - np.floor(t)
        assert ((f > 0.45) & (f < 0.5)).sum() >= 5 and ((f > 0.5) & (f < 0.55)).sum() >= 5
    assert counts[5] >= 50 and counts[0] >= 50
    # reference positions the unguarded reference sample would have read outside the level for
    assert ((c["u"] < 0) | (c["u"] > W - 1) | (c["v"] < 0) | (c["v"] > H - 1)).sum() >= 5
    # idepth on both sides of both bounds
    for b in (am.IDEPTH_MIN, am.IDEPTH_MAX):
        d = c["idepth"] - b
        assert ((d > 0) & (d < 1e-2)).sum() >= 5 and ((d < 0) & (d > -1e-2)).sum() >= 5


# ---------------------------------------------------------------------------------------------------------------------------------------
# what single precision does to a case: the numbers DESIGN.md quotes; the device tests take 8 x these, computed by the same functions
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_float32_sensitivity_measurement():
    eps32 = 2.0 ** -24
    for name, n in F32_CASES:
        s1 = am.f32_first_iteration_sensitivity(name, n)
        print(f"float32 sensitivity of the first iteration, {name} n={n}: H {s1['H']:.3e} (scaled {s1['H_scaled']:.3e}) energy {s1['energy']:.3e} pose {s1['pose']:.3e} "
              f"affine {s1['affine']:.3e}")
        # sanity of the measurement itself: single-precision round-off, not zero and not a wrong term.  A residual of a few grey levels is
        # the difference of intensities of ~100 (relative 2^-24 each); energy and H collect ~n such terms with random signs
        assert eps32 / 100 < s1["energy"] < 3e3 * eps32 and eps32 / 100 < s1["H_scaled"] < 3e3 * eps32
        assert 0 < s1["pose"] < 1e-4
    for name, n in F32_FULL_CASES:
        s2 = am.f32_end_state_sensitivity(name, n)
        print(f"oracle on float32-rounded inputs, {name} n={n}: end pose {s2['pose']:.3e} affine {s2['affine']:.3e} energy {s2['energy']:.3e} iterations {s2['iterations']}")
        assert 0 < s2["pose"] < 1e-4 and s2["iterations"][0] == s2["iterations"][1]
