"""The step from the columns of L^-1 (tests/dense_solve_columns_model.py: the arithmetic the device uses for K <= 64, where the
back-substitution rides under the factorisation) against the backward-error criterion of tests/dense_solve_model.py, on the CPU oracle's
systems: it meets cap and working threshold wherever the substitution does, it is exactly 0 where the substitution's step is, and a
column that misses one block row's contribution is rejected."""
import numpy as np
import pytest

import dense_solve_columns_model as cm
import dense_solve_model as dm
from test_dense_solve import _marginal_oracle, _oracle, _sweeps

CASES = [(2, False), (7, False), (8, False), (8, True)]


def _case_sweeps(F, flip_last):
    win = dm.make_case_window(F, flip_last=flip_last)
    ids = [f.frame_id for f in win.frames]
    return _sweeps(_oracle(win), ids)


@pytest.mark.parametrize("F,flip_last", CASES)
def test_column_step_meets_the_criterion(F, flip_last):
    K = 8 * F
    worst, worst_diff = 0.0, 0.0
    for rnd, inputs, lam, _ in _case_sweeps(F, flip_last):
        A, g = dm.assemble64(*inputs, lam)
        L, y, inv = cm.factor(A, g)
        x_cols = cm.columns_step_from_factor(L, y, inv)
        x_sub = cm.substitution_step(L, y, inv)
        w, _, m = dm.check_step(inputs, lam, x_cols, f"columns F={F} flip={flip_last} round {rnd}")
        # exactly 0 where the substitution's step is, at the same entries
        assert np.array_equal(x_cols == 0, x_sub == 0), (F, lam)
        if flip_last:
            assert np.array_equal(np.flatnonzero(m.empty), np.arange(K - 8, K - 2))   # the six pose rows of the flipped keyframe
            assert np.all(x_cols[K - 8:K - 2] == 0)
            assert all(m.r[i] == 0 for i in range(K - 8, K - 2))
        d = np.sqrt(dm.scale_terms(inputs[0], inputs[2], inputs[4], lam))
        worst = max(worst, w)
        worst_diff = max(worst_diff, np.linalg.norm(d * (x_cols - x_sub)) / np.linalg.norm(d * x_sub))
    print(f"DENSE_SOLVE_COLUMNS cpu F={F} flip={int(flip_last)} omega={worst / dm.U:.2f}u cap={dm.cap(K) / dm.U:.0f}u "
          f"|D(x_cols - x_sub)|/|D x_sub|={worst_diff:.2e}")


def test_column_step_meets_the_criterion_with_a_marginal_prior():
    o, ids = _marginal_oracle("four")
    assert o.K == 32
    o.begin()
    o.linearize()
    inputs = dm.read_inputs(o, ids)
    assert np.abs(inputs[4]).max() > 0 and np.abs(inputs[4] @ inputs[6]).max() > 0   # H_m and H_m eps are in the system
    for lam in dm.LAMBDAS:
        A, g = dm.assemble64(*inputs, lam)
        L, y, inv = cm.factor(A, g)
        x_cols = cm.columns_step_from_factor(L, y, inv)
        dm.check_step(inputs, lam, x_cols, "columns, marginal four")
        assert np.array_equal(x_cols == 0, cm.substitution_step(L, y, inv) == 0)


@pytest.mark.parametrize("F", [2, 7, 8])
def test_a_column_that_misses_a_block_row_is_rejected(F):
    """the fault: column 0 leaves the contribution of its own block out of the last block row.  The model's correct step passes on the same
    inputs, so what is rejected is the fault."""
    for rnd, inputs, lam, _ in _case_sweeps(F, False):
        A, g = dm.assemble64(*inputs, lam)
        x_ref = dm.lapack_step(*inputs, lam)
        thr = min(dm.working_threshold(dm.measure(*inputs, lam, x_ref).omega), dm.cap(8 * F))
        assert dm.measure(*inputs, lam, cm.columns_step(A, g)).omega <= thr
        assert dm.measure(*inputs, lam, cm.columns_step(A, g, skip=(0, 0, F - 1))).omega > thr, (F, lam)
