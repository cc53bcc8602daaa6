"""The criterion of tests/dense_solve_model.py itself, on the CPU: the reference solvers (the oracle's calculate_step — pivoted L D L^T of
the Jacobi-scaled system — and a float64 LAPACK Cholesky) meet it on every window and damping tests/test_gpu_dense_solve.py runs, so it
is attainable on these inputs by the reference alone; deliberately wrong solves do not; and omega does not move under the diagonal
scaling the device skips."""
import numpy as np
import pytest

import dense_solve_model as dm
from dsopp_amd import synthetic as syn
from test_marginalization import _build


def _oracle(win):
    from oracle import pyoracle as po
    return syn.load_window(po.OracleWindow(po.default_pba_options()), win)


def _sweeps(o, ids):
    """(inputs, lambda, oracle step) for the damping sweep at the initial state and once more from the moved state (eps != 0)"""
    o.begin()
    o.linearize()
    for rnd in range(2):
        inputs = dm.read_inputs(o, ids)
        for lam in dm.LAMBDAS:
            yield rnd, inputs, lam, o.calculate_step(lam)
        if rnd == 0:
            o.calculate_step(1e-5)
            o.calculate_energy()
            o.accept_step()
            o.linearize()


def _marginal_oracle(case):
    from oracle import pyoracle as po
    n_frames, n0 = (5, 4) if case == "four" else (10, 9)
    win = dm.make_marginal_window(n_frames)
    o = _build(po.OracleWindow, po.default_pba_options(), win, n0, marg_frame=1, marg_points=1)
    ids = [f.frame_id for i, f in enumerate(win.frames[:n0 + 1]) if i != 1]
    return o, ids


@pytest.mark.parametrize("F", dm.WINDOW_FRAMES)
def test_reference_solvers_meet_the_criterion(F):
    win = dm.make_case_window(F)
    ids = [f.frame_id for f in win.frames]
    o = _oracle(win)
    worst = [0.0, 0.0]
    for rnd, inputs, lam, x_oracle in _sweeps(o, ids):
        w_o, w_l, _ = dm.check_step(inputs, lam, x_oracle, f"oracle F={F} round {rnd}")
        assert w_l <= dm.cap(8 * F), (F, lam, w_l)
        if rnd == 1:
            assert np.abs(inputs[6]).max() > 0   # the second sweep starts from a moved state
        worst = [max(worst[0], w_o), max(worst[1], w_l)]
    print(f"DENSE_SOLVE cpu F={F} omega_oracle={worst[0] / dm.U:.2f}u omega_lapack={worst[1] / dm.U:.2f}u cap={dm.cap(8 * F) / dm.U:.0f}u")


@pytest.mark.parametrize("case", ["four", "ten"])
def test_reference_solvers_meet_the_criterion_with_a_marginal_prior(case):
    o, ids = _marginal_oracle(case)
    assert o.K == 8 * len(ids) == (32 if case == "four" else 72)
    o.begin()
    o.linearize()
    inputs = dm.read_inputs(o, ids)
    assert np.abs(inputs[4]).max() > 0 and np.abs(inputs[4] @ inputs[6]).max() > 0   # H_m and H_m eps are in the system
    for lam in dm.LAMBDAS:
        w_o, w_l, _ = dm.check_step(inputs, lam, o.calculate_step(lam), f"oracle marginal {case}")
        assert w_l <= dm.cap(o.K)


def test_reference_solvers_meet_the_criterion_with_a_frame_without_information():
    win = dm.make_case_window(9, flip_last=True)
    ids = [f.frame_id for f in win.frames]
    o = _oracle(win)
    o.begin()
    o.linearize()
    inputs = dm.read_inputs(o, ids)
    for lam in dm.LAMBDAS:
        x = o.calculate_step(lam)
        _, w_l, m = dm.check_step(inputs, lam, x, "oracle, flipped keyframe")
        assert w_l <= dm.cap(72)
        assert np.array_equal(np.flatnonzero(m.empty), np.arange(64, 70))   # the six pose rows of the flipped keyframe: nothing added
        assert np.all(x[64:70] == 0)


@pytest.mark.parametrize("F", dm.WINDOW_FRAMES)
def test_wrong_solves_are_rejected(F):
    """every fault below is far inside the parity bars of the suite (1e-9 absolute on a step of 1e-2 .. 1e-1)"""
    win = dm.make_case_window(F)
    ids = [f.frame_id for f in win.frames]
    K = 8 * F
    o = _oracle(win)
    floor = 64
    for rnd, inputs, lam, _ in _sweeps(o, ids):
        A, g = dm.assemble64(*inputs, lam)
        x_ref = dm.lapack_step(*inputs, lam)
        thr = min(dm.working_threshold(dm.measure(*inputs, lam, x_ref).omega), dm.cap(K))
        # the model's own correct solve passes: what is rejected below is the fault, not the model
        assert dm.measure(*inputs, lam, dm.cholesky_step(A, g)).omega <= thr
        # pivot reciprocals off by 2^-23 (a hardware estimate without its Newton steps) and by 2^-40
        ratios = {p: dm.measure(*inputs, lam, dm.cholesky_step(A, g, recip_factor=1.0 + 2.0 ** -p)).omega / thr for p in range(23, 53)}
        assert ratios[23] > 1 and ratios[40] > 1, (F, lam, ratios[23], ratios[40])
        floor = min(floor, next(p for p in range(23, 54) if p == 53 or ratios[p] <= 1) - 1)
        # one entry of the correct step off by 1e-11 relative (the entry that weighs most in the criterion's own scale)
        s = dm.scale_terms(inputs[0], inputs[2], inputs[4], lam)
        j = int(np.argmax(np.sqrt(s) * np.abs(x_ref)))
        x_bad = x_ref.copy()
        x_bad[j] *= 1.0 + 1e-11
        assert dm.measure(*inputs, lam, x_bad).omega > thr, (F, lam, j)
        # the right-hand-side row left out of the update by block column 0
        assert dm.measure(*inputs, lam, dm.cholesky_step(A, g, skip_rhs_update_of_block=0)).omega > thr, (F, lam)
    print(f"DENSE_SOLVE cpu F={F} every pivot perturbation 2^-p with p <= {floor} is rejected at every damping")


def test_omega_is_invariant_under_diagonal_scaling():
    """16 unknowns (the 2-frame window) with a prior and a moved state added; d_i are powers of two, so that the scaled float64 inputs
    are the exact scalings and only the criterion is under test"""
    win = dm.make_case_window(2)
    o = _oracle(win)
    o.begin()
    o.linearize()
    H_pp, b_pp, H_schur, b_schur, _, _, _ = dm.read_inputs(o, [f.frame_id for f in win.frames])
    rng = np.random.default_rng(7)
    J = rng.normal(size=(20, 16)) * 1e3
    H_m, b_m, eps = J.T @ J, rng.normal(size=16) * 1e4, rng.normal(size=16) * 1e-3
    lam = 1e-2
    x = dm.lapack_step(H_pp, b_pp, H_schur, b_schur, H_m, b_m, eps, lam)
    x[int(np.argmax(np.abs(x)))] *= 1 + 1e-8    # a measurable omega, far above the rounding of the measure itself
    w0 = dm.measure(H_pp, b_pp, H_schur, b_schur, H_m, b_m, eps, lam, x).omega
    assert w0 > 1e3 * dm.U
    d = 2.0 ** rng.integers(-20, 21, 16)
    D = np.outer(d, d)
    w1 = dm.measure(H_pp * D, b_pp * d, H_schur * D, b_schur * d, H_m * D, b_m * d, eps / d, lam, x / d).omega
    assert abs(w1 - w0) <= 1e-12 * w0, (w0, w1)


def test_both_extended_precisions_agree():
    """the mpmath route (hosts without an 80-bit long double) gives the figure of the long-double route (trivially so on such a host)"""
    win = dm.make_case_window(2)
    o = _oracle(win)
    o.begin()
    o.linearize()
    inputs = dm.read_inputs(o, [f.frame_id for f in win.frames])
    x = o.calculate_step(1e-5)
    a, b = dm.measure(*inputs, 1e-5, x).omega, dm.measure(*inputs, 1e-5, x, force="mpmath").omega
    assert abs(a - b) <= 1e-3 * b, (a, b)
