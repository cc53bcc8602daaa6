"""The dense solve whose back-substitution rides under the factorisation (pba_solve_kernels.hpp: choleskyAugmentedImpl with the column
substitution, K <= 64) in the two kernels that carry it — the fused reduce + solve launch (reduceSolveFusedKernel<256>: seven helper
waves) and the stage API's assembleSolveKernel (three helper waves) — against each other and against an independent reference on the
device: the two-launch path's solveCombinedKernel<256>, which keeps backSubstituteWave behind the factorisation
(DSOPP_HIP_FUSED_REDUCE_SOLVE=0, read once per process: a fresh child).  The three first steps of one window must agree pairwise within
the bound two backward-stable solutions of one system obey (tests/test_gpu_dense_solve.py), a keyframe without information must get a
pose step of exactly 0 from all three, and two staged solves of a deterministic window — the same system twice through the column
substitution — must give the same bits.  tests/test_gpu_dense_solve.py holds the same routine to cap and working threshold through the
stage API; tests/dense_solve_columns_model.py states its arithmetic.

320 x 240 windows with 80 landmarks per keyframe (dense_solve_model.make_case_window), each the smallest at which a path exists:
   F = 2            one look-ahead step: a column advances by exactly one off-diagonal block row; most helper waves carry no column
   F = 7            production size: 56 columns, every helper lane of the fused launch busy
   F = 8            64 columns: a second column block on a helper wave of the fused launch, a third in assembleSolveKernel; the
                    right-hand-side row beyond lane 63
   F = 8, flipped   zero pivots through the fused loop's kernels (the last keyframe looks the other way)
   marginal prior   the 4-frame window of tests/test_marginalization.py, K = 32, in the fused loop
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import dense_solve_model as dm
from test_gpu_dense_solve import _assert_within_perturbation_bound, _fused_first_step, _staged_first_step
from test_marginalization import _build

pytestmark = pytest.mark.gpu

CASES = [(2, False), (7, False), (8, False), (8, True)]
INPUT_NAMES = ("H_pp", "b_pp", "H_schur", "b_schur", "H_m", "b_m", "eps")


def _marginal_first_steps():
    """the 4-frame window with a marginal prior: the first step of the loop and of the stages from ONE built window (snapshot / restore),
    as differences of the frame states: (loop step, staged step, inputs, lambda)"""
    from dsopp_amd import capi
    win = dm.make_marginal_window(5)
    g = _build(capi.HipWindow, capi.default_pba_options(), win, 4, marg_frame=1, marg_points=1)
    ids = [f.frame_id for i, f in enumerate(win.frames[:5]) if i != 1]
    assert g.K == 32 and np.abs(g.get_marginalized()[0]).max() > 0
    state = lambda: np.concatenate([g.get_frame_state(fid)[2] for fid in ids])
    g.snapshot()
    eps0 = state()
    g.set_max_iterations(1)
    _, it, _ = g.optimize()
    assert it == 1
    d_loop = state() - eps0
    g.restore()
    g.set_deterministic(True)
    lam = 1.0 / g.options.initial_trust_region_radius
    g.begin()
    g.calculate_energy()
    g.linearize()
    inputs = dm.read_inputs(g, ids)
    g.calculate_step(lam)
    g.calculate_energy()
    g.accept_step()
    d_staged = state() - eps0
    g.close()
    return d_loop, d_staged, inputs, lam


_CHILD = r"""
import sys
import numpy as np
import dense_solve_model as dm
from test_gpu_dense_solve import _fused_first_step
from test_gpu_dense_solve_columns import CASES, INPUT_NAMES, _marginal_first_steps
out = {}
for F, flip in CASES:
    out[f"eps_{F}_{int(flip)}"], _ = _fused_first_step(dm.make_case_window(F, flip_last=flip), False)
d_loop, d_staged, inputs, lam = _marginal_first_steps()
out.update(marginal_loop=d_loop, marginal_staged=d_staged, marginal_lam=lam, **{f"marginal_{n}": v for n, v in zip(INPUT_NAMES, inputs)})
np.savez(sys.argv[1], **out)
print("columns cases ok")
"""


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    """every case once more on the two-launch path, in one fresh child process"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path_factory.mktemp("dense_solve_columns") / "split.npz")
    env = dict(os.environ, DSOPP_HIP_FUSED_REDUCE_SOLVE="0", PYTHONPATH=os.pathsep.join([root, os.path.join(root, "tests")]))
    r = subprocess.run([sys.executable, "-c", _CHILD, path], cwd=root, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "columns cases ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(path)


def _live(inputs, *steps):
    """the system without the rows nothing was added to (their unknowns are no equations: asserted to be exactly 0 by the caller), so that
    the perturbation bound's scaling D has no zero"""
    H_pp, b_pp, H_schur, b_schur, H_m, b_m, eps = inputs
    live = dm.scale_terms(H_pp, H_schur, H_m, 0.0) > 0
    sub = lambda M: M[np.ix_(live, live)]
    return (sub(H_pp), b_pp[live], sub(H_schur), b_schur[live], sub(H_m), b_m[live], eps[live]), [s[live] for s in steps], live


@pytest.mark.parametrize("F,flip", CASES)
def test_fused_split_and_staged_first_steps_agree(split, F, flip):
    win = dm.make_case_window(F, flip_last=flip)
    K = 8 * F
    eps_fused, poses = _fused_first_step(win, False)
    eps_split = split[f"eps_{F}_{int(flip)}"]
    eps_staged, _, inputs, lam = _staged_first_step(win, True)
    steps = {"fused": eps_fused, "split": eps_split, "staged": eps_staged}
    for name, e in steps.items():
        assert e.shape == (K,) and np.all(np.isfinite(e)), name
        assert np.abs(e).max() > 0, name
    assert np.all(np.isfinite(poses))
    sub_inputs, (sf, ss, sg), live = _live(inputs, eps_fused, eps_split, eps_staged)
    if flip:
        # the six pose rows of the flipped keyframe: nothing was added to them; every kernel leaves their step at exactly 0
        assert np.array_equal(np.flatnonzero(~live), np.arange(K - 8, K - 2))
        for name, e in steps.items():
            assert np.all(e[K - 8:K - 2] == 0), name
    else:
        assert np.all(live)
    _assert_within_perturbation_bound(sf, sg, sub_inputs, lam, f"columns F={F} flip={int(flip)} fused against staged")
    _assert_within_perturbation_bound(ss, sg, sub_inputs, lam, f"columns F={F} flip={int(flip)} split against staged")
    _assert_within_perturbation_bound(sf, ss, sub_inputs, lam, f"columns F={F} flip={int(flip)} fused against split")


@pytest.mark.parametrize("F,flip", CASES)
def test_two_solves_of_a_deterministic_window_give_identical_bits(F, flip):
    """Deterministic summation gives assembleSolveKernel the same system twice, and that kernel substitutes by columns on its three helper
    waves: a race in the in-column exchange, or an order of the arithmetic that depended on timing, would show as differing bits.  (The
    fused launch cannot stand here: its system is summed with atomics.  A deterministic window's LOOP runs solveCombinedKernel<256>,
    which keeps backSubstituteWave, so the staged step is the one that runs the routine.)  The systems are compared too, so that a
    difference in the step cannot come from the build."""
    win = dm.make_case_window(F, flip_last=flip)
    eps_a, poses_a, inputs_a, lam_a = _staged_first_step(win, True)
    eps_b, poses_b, inputs_b, lam_b = _staged_first_step(win, True)
    assert lam_a == lam_b and all(np.array_equal(u, v) for u, v in zip(inputs_a, inputs_b))
    assert np.abs(eps_a).max() > 0
    assert np.array_equal(eps_a, eps_b) and np.array_equal(poses_a, poses_b)
    if flip:
        assert np.all(eps_a[8 * F - 8:8 * F - 2] == 0)


def test_marginal_prior_in_the_fused_loop(split):
    """K = 32 with H_m in the matrix and b_m + H_m eps in the right-hand side, from a moved state: the loop's first step (fused launch here,
    the two launches in the child) against the staged step of the same built window"""
    d_loop, d_staged, inputs, lam = _marginal_first_steps()
    assert np.abs(inputs[4]).max() > 0 and np.abs(inputs[4] @ inputs[6]).max() > 0   # the case cannot pass empty
    assert np.all(np.isfinite(d_loop)) and np.abs(d_loop).max() > 0
    _assert_within_perturbation_bound(d_loop, d_staged, inputs, lam, "columns marginal fused against staged")
    c_inputs = tuple(split[f"marginal_{n}"] for n in INPUT_NAMES)
    assert np.all(np.isfinite(split["marginal_loop"])) and np.abs(split["marginal_loop"]).max() > 0
    _assert_within_perturbation_bound(split["marginal_loop"], split["marginal_staged"], c_inputs, float(split["marginal_lam"]),
                                      "columns marginal split against staged")
