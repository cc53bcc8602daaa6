"""The window's dense solve — choleskyAugmented + backSubstituteWave of pba_solve_kernels.hpp, behind assembleSolveKernel (stage API,
marginalisation, lm_mode 1) and solveCombinedKernel<256>, <256, kMaxCombCopies>, <512> (the fused loop) — against the backward-error
criterion of tests/dense_solve_model.py: a residual in extended precision with a cap that follows from the algorithm and a working
threshold measured on a LAPACK solve of the same inputs inside each case.  No figure here comes from the kernel, from the oracle's
solver or from the conditioning of the reduced system (tests/test_dense_solve.py shows on the CPU that the references meet the
criterion on these very windows and that wrong solves do not).

Window sizes (320 x 240, 80 landmarks per keyframe), each the smallest at which a path of the solve exists:
   F   K / N     what only this size reaches
   2   16 / 17   one look-ahead step, minimum window
   7   56 / 57   production size, every row inside one wave
   8   64 / 65   the right-hand-side row alone beyond lane 63 (the r2 loop of the panel runs for one row); the single-register
                 back substitution at its largest size
   9   72 / 73   first K > 64: two-register back substitution with one upper block; solveCombinedKernel<512> in the fused loop
  12   96 / 97   the size of the C4 configuration
  16  128 / 129  capacity; the r2 loop runs twice
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import dense_solve_model as dm
from dsopp_amd import synthetic as syn
from test_marginalization import _build

pytestmark = pytest.mark.gpu


def _window(win, deterministic=False):
    from dsopp_amd import capi
    g = syn.load_window(capi.HipWindow(capi.default_pba_options()), win)
    g.set_deterministic(deterministic)
    return g


def _sweep(g, ids, label, rows=None):
    """the damping sweep on the current linearisation: every step finite, under the cap and the working threshold, and stored negated
    in the frame states bit for bit.  Returns (largest omega, largest omega of the LAPACK solve)."""
    inputs = dm.read_inputs(g, ids)
    worst = [0.0, 0.0]
    for lam in dm.LAMBDAS:
        x = g.calculate_step(lam)
        w, wl, m = dm.check_step(inputs, lam, x, f"{label} lambda={lam:g}")
        stored = np.concatenate([g.get_frame_state(fid)[3] for fid in ids])
        assert np.array_equal(-x, stored), (label, lam)
        if rows is not None:
            rows(m, x)
        worst = [max(worst[0], w), max(worst[1], wl)]
    return worst, inputs


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("F", dm.WINDOW_FRAMES)
def test_stage_step_meets_the_backward_error_bound(F, deterministic):
    win = dm.make_case_window(F)
    ids = [f.frame_id for f in win.frames]
    g = _window(win, deterministic)
    g.begin()
    g.linearize()
    w0, _ = _sweep(g, ids, f"F={F} det={deterministic} initial state")
    g.calculate_step(1e-5)
    g.calculate_energy()
    g.accept_step()
    g.linearize()
    w1, inputs = _sweep(g, ids, f"F={F} det={deterministic} moved state")
    assert np.abs(inputs[6]).max() > 0
    g.close()
    print(f"DENSE_SOLVE gpu F={F} det={int(deterministic)} omega_gpu={max(w0[0], w1[0]) / dm.U:.2f}u "
          f"omega_lapack={max(w0[1], w1[1]) / dm.U:.2f}u cap={dm.cap(8 * F) / dm.U:.0f}u")


@pytest.mark.parametrize("case", ["four", "ten"])
def test_stage_step_with_a_marginal_prior(case):
    """H_m in the matrix and b_m + H_m eps in the right-hand side (use_marginal: a K-long dot product per thread): the 4-frame case of
    tests/test_marginalization.py, and 9 keyframes + 1 with one marginalised, which leaves F = 9 — the prior in a K > 64 system"""
    from dsopp_amd import capi
    n_frames, n0 = (5, 4) if case == "four" else (10, 9)
    win = dm.make_marginal_window(n_frames)
    g = _build(capi.HipWindow, capi.default_pba_options(), win, n0, marg_frame=1, marg_points=1)
    ids = [f.frame_id for i, f in enumerate(win.frames[:n0 + 1]) if i != 1]
    assert g.K == 8 * len(ids) == (32 if case == "four" else 72)
    g.begin()
    g.linearize()
    worst, inputs = _sweep(g, ids, f"marginal prior, {case}")
    H_m, eps = inputs[4], inputs[6]
    assert np.abs(H_m).max() > 0 and np.abs(H_m @ eps).max() > 0   # the case cannot pass empty
    g.close()
    print(f"DENSE_SOLVE gpu marginal {case} omega_gpu={worst[0] / dm.U:.2f}u omega_lapack={worst[1] / dm.U:.2f}u")


def test_stage_step_with_a_frame_without_information():
    """9 keyframes, the last one looks the other way: its six pose rows are empty (nothing was added to them: zero denominator), the
    zero-pivot guard inside the r2 loop and the two-register sweep must leave r_i == 0 and a pose step of exactly 0 there, and every
    other row meets the thresholds"""
    win = dm.make_case_window(9, flip_last=True)
    ids = [f.frame_id for f in win.frames]
    g = _window(win)
    g.begin()
    g.linearize()

    def rows(m, x):
        assert np.array_equal(np.flatnonzero(m.empty), np.arange(64, 70))
        assert all(m.r[i] == 0 for i in range(64, 70))
        assert np.all(x[64:70] == 0)

    worst, _ = _sweep(g, ids, "flipped keyframe", rows)   # (check_step: every row with a denominator is under both thresholds)
    g.close()
    print(f"DENSE_SOLVE gpu flipped omega_gpu={worst[0] / dm.U:.2f}u omega_lapack={worst[1] / dm.U:.2f}u")


# ---- the fused loop's solve kernels do the staged arithmetic

def _fused_first_step(win, deterministic):
    """one iteration of the fused loop: (eps, poses)"""
    g = _window(win, deterministic)
    g.set_max_iterations(1)
    _, it, _ = g.optimize()
    assert it == 1
    ids = [f.frame_id for f in win.frames]
    eps = np.concatenate([g.get_frame_state(fid)[2] for fid in ids])
    poses = np.concatenate([np.concatenate(g.get_pose(fid)) for fid in ids])
    g.close()
    return eps, poses


def _staged_first_step(win, deterministic):
    """the same iteration through the stage API: (eps, poses, inputs, lambda)"""
    g = _window(win, deterministic)
    ids = [f.frame_id for f in win.frames]
    lam = 1.0 / g.options.initial_trust_region_radius
    g.begin()
    g.calculate_energy()
    g.linearize()
    inputs = dm.read_inputs(g, ids)
    g.calculate_step(lam)
    g.calculate_energy()
    g.accept_step()
    eps = np.concatenate([g.get_frame_state(fid)[2] for fid in ids])
    poses = np.concatenate([np.concatenate(g.get_pose(fid)) for fid in ids])
    g.close()
    return eps, poses, inputs, lam


def _assert_within_perturbation_bound(eps_a, eps_b, inputs, lam, label):
    """two solutions of backward error <= tau of one system: || D (x_A - x_B) ||_2 <= 2 kappa_2(D^-1 A D^-1) n tau || D x_B ||_2,
    D = diag(sqrt(s)), tau the working threshold of the case, kappa_2 from the staged window's system.  (x = -eps: the first step from
    eps = 0.)"""
    A, _ = dm.assemble64(*inputs, lam)
    s = dm.scale_terms(inputs[0], inputs[2], inputs[4], lam)
    d = np.sqrt(s)
    assert np.all(d > 0)
    kappa = np.linalg.cond(A / np.outer(d, d), 2)
    tau = dm.working_threshold(dm.measure(*inputs, lam, dm.lapack_step(*inputs, lam)).omega)
    n = len(eps_b) + 1
    lhs = np.linalg.norm(d * (eps_a - eps_b))
    rhs = 2.0 * kappa * n * tau * np.linalg.norm(d * eps_b)
    print(f"DENSE_SOLVE gpu {label}: identical={np.array_equal(eps_a, eps_b)} |D dx|={lhs:.3e} bound={rhs:.3e} kappa={kappa:.3e} "
          f"max|dx|={np.abs(eps_a - eps_b).max():.3e}")
    assert lhs <= rhs, (label, lhs, rhs, kappa)


@pytest.mark.parametrize("F", [7, 9])
def test_fused_solve_kernels_do_the_staged_arithmetic(F):
    """solveCombinedKernel<256> (7 keyframes) and <512> (9) against assembleSolveKernel, deterministic summation on both sides.  They
    are NOT bit-identical: the fused loop sums the combined system A = H_pp (1 + lambda) - H_schur / (1 + lambda) term by term, each
    term scaled before it is added, the stages scale the finished sums (dense-solve row of the test table) — so the bound two
    backward-stable solutions of one system obey is asserted."""
    win = dm.make_case_window(F)
    eps_a, poses_a = _fused_first_step(win, True)
    eps_b, poses_b, inputs, lam = _staged_first_step(win, True)
    assert np.all(np.isfinite(eps_a)) and np.all(np.isfinite(poses_a))
    _assert_within_perturbation_bound(eps_a, eps_b, inputs, lam, f"fused against staged F={F}")
    # the pose is T0 exp(eps) on both sides: it moves by no more than the state did (unit quaternion, first-order in eps)
    assert np.abs(poses_a - poses_b).max() <= 4.0 * np.abs(eps_a - eps_b).max() + 8 * dm.U * np.abs(poses_b).max()


_COPIES_SCRIPT = r"""
import sys
import numpy as np
import dense_solve_model as dm
from dsopp_amd import capi, synthetic as syn
win = dm.make_case_window(7)
g = syn.load_window(capi.HipWindow(capi.default_pba_options()), win)
g.set_max_iterations(1)
_, it, _ = g.optimize()
eps = np.concatenate([g.get_frame_state(f.frame_id)[2] for f in win.frames])
g.close()
np.savez(sys.argv[1], eps=eps, it=it)
print("copies ok")
"""


def test_fused_solve_kernel_that_adds_the_copies_does_the_staged_arithmetic(tmp_path):
    """solveCombinedKernel<256, kMaxCombCopies>: the reduction spreads its atomics over several copies of the combined system and the
    solve adds them while loading (forced on by DSOPP_HIP_COMB_COPIES_MIN_CHUNKS=1, read once per process: a fresh child).  That path
    sums with atomics, so the perturbation bound applies, not equality."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / "copies.npz")
    env = dict(os.environ, DSOPP_HIP_COMB_COPIES_MIN_CHUNKS="1", PYTHONPATH=os.pathsep.join([root, os.path.join(root, "tests")]))
    r = subprocess.run([sys.executable, "-c", _COPIES_SCRIPT, path], cwd=root, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "copies ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    res = np.load(path)
    assert int(res["it"]) == 1 and np.all(np.isfinite(res["eps"]))
    eps_b, _, inputs, lam = _staged_first_step(dm.make_case_window(7), True)
    _assert_within_perturbation_bound(res["eps"], eps_b, inputs, lam, "fused with copies against staged F=7")
