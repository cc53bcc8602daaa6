"""tests/activation_model.py against the CPU oracle on every scene of tests/activation_scenes.py, and the scenes against what they were built
to reach.  No GPU: the model is what tests/test_gpu_activation_edges.py holds the device to, so it is pinned here first — on the oracle
(a C++ restatement of the same reference code, in binary64) and, for the designed scenes, on statuses written out by hand."""
from fractions import Fraction

import numpy as np
import pytest

import activation_model as am
import activation_scenes as asc

A, S, D = am.ACTIVATE, am.SKIP, am.DELETE
# refined inverse depths, model (binary64) against oracle (binary64): two restatements of one computation that differ in the order of a few
# sums and in how the relative pose is composed.  Measured over all refinement scenes: 4.774e-15 relative (refine_F2); the bar is 10 x that
REFINED_RTOL = 5e-14


def _oracle(sc):
    from oracle import pyoracle as po
    fo = asc.oracle_frames(sc["frames"])
    st, n, d = po.activate_landmarks(fo, sc["intr"], sc["sigma"], sc["desired"], sc["dist0"], refine=sc["refine"], mask_sparsity_newest=sc["ms"])
    return fo, st, n, d


def _check_against_oracle(sc, m):
    fo, st, n, d = _oracle(sc)
    assert n == m.n_active
    assert d == m.distance, (d, m.distance)
    assert len(st) == len(m.statuses)
    for k, (a, b) in enumerate(zip(st, m.statuses)):
        assert np.array_equal(a, b), (k, np.flatnonzero(a != b), a[a != b], b[a != b])
    worst = 0.0
    for f, state in zip(fo[:-1], m.states):
        if state is None:
            assert len(f["immature"]["status"]) == 0
            continue
        assert np.array_equal(f["immature"]["status"], state["status"])
        for key in ("idepth_min", "idepth_max"):
            a, b = f["immature"][key], state[key]
            worst = max(worst, float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(a)), initial=0.0)))
    return worst


def test_scene_lists_are_complete():
    assert list(asc.scenes("selection")) == asc.SELECTION_NAMES
    assert list(asc.scenes("refinement")) == asc.REFINEMENT_NAMES
    for sc in asc.scenes("selection").values():
        for f in sc["frames"]:
            assert f["pixelinfo"].shape[0] <= 98 and f["pixelinfo"].shape[1] <= 130
        if sc["exact"]:   # the regulator leaves the distance alone
            assert asc.model(sc).distance == sc["dist0"]


@pytest.mark.parametrize("name", asc.SELECTION_NAMES)
def test_selection_model_equals_oracle_and_exact_arithmetic(name):
    sc = asc.scenes("selection")[name]
    m = asc.model(sc)
    assert _check_against_oracle(sc, m) == 0.0   # no refinement: the intervals are untouched
    # the placements are exact in binary64, so rational arithmetic (squared distances against the squared distance) selects the same
    mf = asc.model(sc, scalar=Fraction)
    for a, b in zip(m.statuses, mf.statuses):
        assert np.array_equal(a, b)
    assert (mf.n_active, mf.n_candidates, mf.n_waiting, mf.max_earlier) == (m.n_active, m.n_candidates, m.n_waiting, m.max_earlier)
    ml = asc.model(sc, scalar=np.longdouble)
    for a, b in zip(m.statuses, ml.statuses):
        assert np.array_equal(a, b)


def _flat(m):
    return np.concatenate(m.statuses).tolist()


def test_tie_scenes_by_hand():
    """candidates: the 3-4-5 pair, a coincident pair, then one on each active landmark: plain, outlier, marginalised, negative idepth,
    idepth 1010, -5e-9, +5e-9, outlier and marginalised"""
    sel = asc.scenes("selection")
    on_active = [S, A, A, A, A, S, S, A]   # only a counted AND kept active landmark blocks; the flushed +-5e-9 are both
    assert _flat(asc.model(sel["ties_d5"])) == [A, A, A, S] + on_active            # exactly the distance apart: strict <, not a neighbour
    assert _flat(asc.model(sel["ties_d5prev"])) == [A, A, A, S] + on_active
    assert _flat(asc.model(sel["ties_d5next"])) == [A, S, A, S] + on_active
    assert _flat(asc.model(sel["ties_d0"])) == [A] * 12                             # sqrt(0) < 0 is false: nothing is ever a neighbour
    for name in ("ties_d5", "ties_d5next", "ties_d0", "ties_d5prev"):
        assert asc.model(sel[name]).n_active == 4                                   # plain, idepth 1010 and the two flushed ones


def test_chain_cluster_and_workcap_scenes_by_hand():
    sel = asc.scenes("selection")
    for name in ("chain_forward", "chain_reverse"):
        m = asc.model(sel[name])
        assert m.n_candidates >= 300 and m.n_waiting == m.n_candidates - 1 and len(m.statuses) == 3
        assert _flat(m) == [A, S] * (m.n_candidates // 2)                           # a path 0.75 d apart: strictly alternating
    m = asc.model(sel["chain_shuffled"])
    assert m.n_candidates >= 300 and m.n_waiting > 200 and set(_flat(m)) == {A, S}
    m = asc.model(sel["cluster_disc"])
    assert _flat(m) == [A] + [S] * 39 and m.max_earlier == 39
    for k in (12, 13):
        m = asc.model(sel["cluster_through_%d" % k])
        assert _flat(m) == [A] + [S] * k + [A] and m.max_earlier == k               # the neighbour list is exactly full / overflows by one
    for n in (8, 9):
        m = asc.model(sel["workcap_%d" % n])
        assert m.n_waiting == n and _flat(m).count(S) == n


def test_grid_mask_status_and_count_scenes_by_hand():
    sel = asc.scenes("selection")
    four_apart = lambda name: _flat(asc.model(sel[name]))[20:22]   # noqa: E731  (the pair exactly 4 apart)
    assert four_apart("grid_d4") == [A, A] and four_apart("grid_d4ulp") == [A, S] and four_apart("grid_d0.5") == [A, A]
    assert asc.model(sel["grid_clamp10"]).distance == 10.0 and asc.model(sel["grid_clamp0"]).distance == 0.0
    assert _flat(asc.model(sel["grid_clamp10"])) == _flat(asc.model(sel["grid_d10"]))
    assert _flat(asc.model(sel["grid_clamp0"])) == [A] * 22
    for name in ("grid_d0.5", "grid_d4", "grid_130x98"):
        assert _flat(asc.model(sel[name]))[:20] == [A, S] * 10                      # every straddling / edge pair: second one skipped
    assert _flat(asc.model(sel["grid_129x96"]))[:20] == [A, S] * 10 and _flat(asc.model(sel["grid_129x96"]))[22] == D
    assert _flat(asc.model(sel["mask_half_hit"])) == [D, A] and _flat(asc.model(sel["mask_half_miss"])) == [A, A]
    # status table, written out: rows status x traced, columns ready, interval 8, uniqueness 3, midpoint 0, edge 4, edge W/2 - 5, outside
    m = asc.model(sel["status_table"])
    got, state = np.concatenate(m.statuses).reshape(14, 7), np.concatenate([s["status"] for s in m.states]).reshape(14, 7)
    for s in range(7):
        for traced in (0, 1):
            row = got[2 * s + traced].tolist()
            if not traced or s in (am.IMM_OUTLIER, am.IMM_DELETE):
                expect = [D] * 7
            elif s == am.IMM_UNINIT:
                expect = [S] * 7
            else:
                not_ready = D if s == am.IMM_OOB else S
                expect = [A, not_ready, not_ready, not_ready, A, A, D]
            assert row == expect, (s, traced, row)
            assert state[2 * s + traced].tolist() == [s if e == S else am.IMM_DELETE for e in expect]
    counts = {name: [(len(f["active_idepth"]), None if f["immature"] is None else len(f["immature"]["status"])) for f in sel["counts_" + name]["frames"][:-1]]
              for name in ("a", "b", "large", "single", "single_1", "single_0", "empty")}
    assert {c[0] for v in counts.values() for c in v} >= {0, 1, 63, 64, 65, 256, 257}
    assert {c[1] for v in counts.values() for c in v} >= {None, 0, 1, 255, 256, 257}
    assert counts["large"][1][1] is None and len(counts["single"]) == 1
    m = asc.model(sel["counts_empty"])
    assert m.n_active == 0 and all(len(s) == 0 for s in m.statuses) and m.distance == 1.5 + (0.0 - 700.0) * 0.001


@pytest.mark.parametrize("name", asc.REFINEMENT_NAMES)
def test_refinement_model_equals_oracle_and_is_stable_in_precision(name):
    sc = asc.scenes("refinement")[name]
    m = asc.model(sc)
    worst = _check_against_oracle(sc, m)
    print(name, "refined inverse depths, model against oracle: %.3e relative" % worst)
    assert worst <= REFINED_RTOL
    # every landmark of the scene takes the same branches in extended precision: none of them sits on a decision
    ml = asc.model(sc, refine_dtype=np.longdouble)
    assert ml.records.keys() == m.records.keys() and len(m.records) > 0
    for key, rec in m.records.items():
        assert ml.records[key] == rec, (key, rec, ml.records[key])
    for a, b in zip(m.statuses, ml.statuses):
        assert np.array_equal(a, b)
    n_frames = len(sc["frames"])
    for f in sc["frames"][:-1]:
        assert f["pixelinfo"].shape[:2] == (asc.RH, asc.RW) and 40 <= len(f["immature"]["status"]) <= 60
    if name.startswith("refine_F"):
        kept = [int((s == A).sum()) for s in m.statuses]
        assert n_frames == int(name[8:]) and kept[0] > 0 and kept[-1] > 0 and (n_frames < 10 or kept[8] > 0), kept
    if name in ("refine_zero_baseline", "refine_masks_zero"):
        assert len(m.records) > 20 and not (np.concatenate(m.statuses) == A).any()
        for f, state in zip(sc["frames"][:-1], m.states):   # deleted: the intervals are untouched
            assert np.array_equal(state["idepth_min"], f["immature"]["idepth_min"]) and np.array_equal(state["idepth_max"], f["immature"]["idepth_max"])
        recs = list(m.records.values())
        assert all(r.zero_hessian and not r.no_valid_at_start for r in recs) if name == "refine_zero_baseline" else all(r.no_valid_at_start for r in recs)
    if name == "refine_wrong_exposure":
        assert sum(r.over_cutoff for r in m.records.values()) > 20
    if name == "refine_huber":
        assert all(r.huber for r in m.records.values())


def test_refinement_scenes_reach_every_branch():
    recs = [r for name in asc.REFINEMENT_NAMES for r in asc.model(asc.scenes("refinement")[name]).records.values()]
    reached = dict(accepted=sum(r.accepted > 0 for r in recs), rejected_then_iterated=sum(r.rejected_then_iterated for r in recs),
                   converged=sum(r.converged for r in recs), no_valid_at_start=sum(r.no_valid_at_start for r in recs),
                   zero_hessian=sum(r.zero_hessian for r in recs), huber=sum(r.huber for r in recs), over_cutoff=sum(r.over_cutoff for r in recs))
    assert all(v > 0 for v in reached.values()), reached
