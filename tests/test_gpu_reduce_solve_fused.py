"""The fused reduce + solve launch of the LM loop (pba_solve_combined.hpp: reduceSolveFusedKernel; pba.hip: launchReduceSolveFused) against
the two launches it replaces.  Every case runs the same seeded window in two fresh child processes (one pair of children per group of cases), one with the switch at its default and
one with DSOPP_HIP_FUSED_REDUCE_SOLVE=0 (read once per process), and compares: iteration counts, residual counts, the status and candidate
status of every residual (what the landmark workgroups' accept / reject writes) and profiles exactly;
energies, poses, affine brightness and inverse depths to the tolerance test_combined_system_accumulated_in_several_copies_equals_the_single_copy
uses (both paths sum with f64 atomics, so bitwise equality is not expected).  The first step is also held against the staged arithmetic with
the perturbation bound of tests/test_gpu_dense_solve.py.

Shapes, each the smallest at which a path exists (320 x 240 case windows of dense_solve_model, 160 x 120 for the landmark counts):
   F = 1, 2, 7, 8            no pair at all / one pair / production size / the last size of the 256-thread solve body
   F = 9                     the 512-thread body in the fused launch
   1, 63, 64, 65, 130 landmarks per frame: a chunk of one, one short of a chunk, a full chunk, a chunk and one, three chunks
   a frame without landmarks, a frame pair without a connection (the pair block that returns early still arrives)
   a marginal prior; force_accept = 0 on a window whose loop rejects; max_iterations 1 and 7; a solve that converges before its budget
   (the launches behind the end of the loop: nobody builds, nobody waits)
   optimize_repeated(21) = three solves enqueued back to back, and two windows solved alternately (the arrival counter's base)
Windows that are not eligible (sharded, deterministic, optimize_idepths = 0, no landmarks, 80 chunks and more) must still run the two
kernels: their profile shows the reduction launches."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dense_solve_model as dm
from test_gpu_dense_solve import _assert_within_perturbation_bound, _staged_first_step

pytestmark = pytest.mark.gpu

_CHILD = r"""
import sys
import numpy as np
import dense_solve_model as dm
from dsopp_amd import capi, synthetic as syn
from test_marginalization import _build

out = {}


def load(win, opts=None, empty_frame=None, skip_pair=None):
    g = capi.HipWindow(opts or capi.default_pba_options())
    intr = win.scene.intrinsics
    for i, f in enumerate(win.frames):
        g.push_frame(f.frame_id, f.timestamp, f.pixelinfo, None, intr, syn.mat_to_params(f.T_w_c_init), f.exposure, f.affine_init, f.fixed, False)
        if i == empty_frame:
            g.set_landmarks(f.frame_id, np.zeros((0, 2)), np.zeros(0), np.zeros((0, 8)), np.zeros(0, dtype=np.uint8))
        else:
            g.set_landmarks(f.frame_id, f.uv, f.idepth_init, f.patch, np.zeros(len(f.uv), dtype=np.uint8))
        for j in range(i):
            for (r, t) in ((j, i), (i, j)):
                if skip_pair is not None and {r, t} == set(skip_pair):
                    continue
                n = 0 if r == empty_frame else len(win.frames[r].uv)
                g.set_connection(win.frames[r].frame_id, win.frames[t].frame_id, np.zeros(n, dtype=np.uint8))
    return g


def record(name, g, ids, result, extra=()):
    e, it, nv = result
    poses = np.concatenate([np.concatenate(g.get_pose(fid)) for fid in ids])     # pose (7) and affine brightness (2) per frame
    eps = np.concatenate([g.get_frame_state(fid)[2] for fid in ids])
    idepths = np.concatenate([g.get_landmarks(fid, with_hpib=False)["idepth"] for fid in ids] + [np.zeros(0)])
    # status and candidate status of every residual list there is (an ordered pair without a connection has none: the call fails)
    st = [np.zeros(0, dtype=np.uint8)]
    for r in ids:
        for t in ids:
            if r != t:
                try:
                    res = g.get_residuals(r, t)
                except capi.HipError:
                    continue
                st += [res["status"], res["candidate"]]
    prof = g.get_profile()
    out[name] = (e, it, nv, poses, idepths, eps, prof["schur"][1], prof["assemble_solve"][1], np.concatenate(st), prof["sweep_energy"][1]) + tuple(extra)


def run(name, win, opts=None, max_iterations=None, prepare=None, **kw):
    g = load(win, opts, **kw)
    if prepare:
        prepare(g)
    if max_iterations is not None:
        g.set_max_iterations(max_iterations)
    g.set_profiling(True)
    record(name, g, [f.frame_id for f in win.frames], g.optimize())
    g.close()


GROUP = sys.argv[2]
four = lambda: syn.make_window(num_frames=4, num_points=320, width=320, height=240, seed=31)

if GROUP == "frames":
    for F in (1, 2, 7, 8, 9):
        run(f"frames{F}", dm.make_case_window(F))

if GROUP == "landmarks":
    for n in (1, 63, 64, 65, 130):
        run(f"landmarks{n}", syn.make_window(num_frames=3, num_points=3 * n, width=160, height=120, seed=200 + n))

if GROUP == "topology":
    run("empty_frame", four(), empty_frame=2)
    run("missing_pair", four(), skip_pair=(1, 3))
    # a marginal prior (the window of tests/test_marginalization.py: four frames solved, one marginalised with a third of another's landmarks)
    mwin = dm.make_marginal_window(5)
    g = _build(capi.HipWindow, capi.default_pba_options(), mwin, 4, marg_frame=1, marg_points=1)
    assert np.abs(g.get_marginalized()[0]).max() > 0
    g.set_profiling(True)
    record("marginal", g, [f.frame_id for i, f in enumerate(mwin.frames[:5]) if i != 1], g.optimize())
    g.close()

if GROUP == "budgets":
    run("first_step7", dm.make_case_window(7), max_iterations=1)
    run("budget7", dm.make_case_window(7), max_iterations=7)
    run("converges", dm.make_case_window(2), max_iterations=20)
    rej = syn.make_window(num_frames=3, num_points=240, width=160, height=120, seed=301)
    run("rejects5", rej, capi.default_pba_options(force_accept=0), max_iterations=5)
    run("rejects6", rej, capi.default_pba_options(force_accept=0), max_iterations=6)

if GROUP == "counter":
    # the counter's base from launch to launch: the windows alone, three solves of 7 iterations enqueued back to back ...
    win7, win8 = dm.make_case_window(7), dm.make_case_window(8)
    run("alone7", win7, max_iterations=7)
    run("alone8", win8)
    g = load(win7)
    g.snapshot()
    g.set_profiling(True)
    n, e_rep = g.optimize_repeated(21)
    record("repeated", g, [f.frame_id for f in win7.frames], (e_rep, n, 0))
    g.close()
    # ... and two windows on one device solved alternately (each from its snapshot)
    a, b = load(win7), load(win8)
    a.snapshot(); b.snapshot()
    a.set_profiling(True); b.set_profiling(True)
    res = []
    for k in range(2):
        for w in (a, b):
            w.restore()
            res.append(w.optimize())
    record("alternate7", a, [f.frame_id for f in win7.frames], res[2], extra=(res[0][0],))
    record("alternate8", b, [f.frame_id for f in win8.frames], res[3], extra=(res[1][0],))
    a.close(); b.close()

if GROUP == "ineligible":
    # windows the fused launch does not take
    run("sharded", four(), prepare=lambda g: g.set_allreduce(lambda ptr, count, stream: 0, 0, 1))
    run("deterministic", four(), prepare=lambda g: g.set_deterministic(True))
    run("fixed_idepths", four(), capi.default_pba_options(optimize_idepths=0))
    run("many_chunks", syn.make_window(num_frames=7, num_points=5200, width=320, height=240, seed=33))
    g = capi.HipWindow(capi.default_pba_options())
    win = four()
    intr = win.scene.intrinsics
    for i, f in enumerate(win.frames[:2]):
        g.push_frame(f.frame_id, f.timestamp, f.pixelinfo, None, intr, syn.mat_to_params(f.T_w_c_init), f.exposure, f.affine_init, f.fixed, False)
        g.set_landmarks(f.frame_id, np.zeros((0, 2)), np.zeros(0), np.zeros((0, 8)), np.zeros(0, dtype=np.uint8))
    g.set_profiling(True)
    record("no_landmarks", g, [f.frame_id for f in win.frames[:2]], g.optimize())
    g.close()

assert out, GROUP
np.savez(sys.argv[1], **{f"{k}_{i}": np.asarray(v) for k, t in out.items() for i, v in enumerate(t)})
print("fused cases ok")
"""

GROUPS = {"frames": ["frames1", "frames2", "frames7", "frames8", "frames9"],
          "landmarks": ["landmarks1", "landmarks63", "landmarks64", "landmarks65", "landmarks130"],
          "topology": ["empty_frame", "missing_pair", "marginal"],
          "budgets": ["first_step7", "budget7", "converges", "rejects5", "rejects6"],
          "counter": ["alone7", "alone8", "repeated", "alternate7", "alternate8"],
          "ineligible": ["sharded", "deterministic", "fixed_idepths", "no_landmarks", "many_chunks"]}
GROUP_OF = {name: group for group, names in GROUPS.items() for name in names}

E, IT, NV, POSES, IDEPTHS, EPS, N_SCHUR, N_SOLVE, STATUSES, N_RESIDUAL_SWEEPS, EXTRA = range(11)


class _Runs:
    """the groups of _CHILD, each run on first use in two fresh child processes: once with the fused launch (the default) and once with the
    two launches.  A group that fails or hangs fails only the tests of its own cases."""

    def __init__(self, tmp):
        self.tmp, self.done = tmp, {}

    def _group(self, group):
        if group not in self.done:
            root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
            res = {}
            for label, switch in (("fused", None), ("split", "0")):
                path = str(self.tmp / f"{group}_{label}.npz")
                env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, os.path.join(root, "tests")]))
                env.pop("DSOPP_HIP_FUSED_REDUCE_SOLVE", None)
                if switch is not None:
                    env["DSOPP_HIP_FUSED_REDUCE_SOLVE"] = switch
                r = subprocess.run([sys.executable, "-c", _CHILD, path, group], cwd=root, env=env, capture_output=True, text=True, timeout=120)
                assert r.returncode == 0 and "fused cases ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
                res[label] = np.load(path)
            self.done[group] = res
        return self.done[group]

    def get(self, which, name, field):
        return self._group(GROUP_OF[name])[which][f"{name}_{field}"]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return _Runs(tmp_path_factory.mktemp("reduce_solve_fused"))


def _assert_same_solve(runs, name):
    a = lambda f: runs.get("fused", name, f)
    b = lambda f: runs.get("split", name, f)
    print(f"FUSED {name}: it {int(a(IT))}/{int(b(IT))} nv {int(a(NV))}/{int(b(NV))} dE/E {abs(float(a(E)) - float(b(E))) / max(abs(float(b(E))), 1e-300):.2e} "
          f"dpose {np.abs(a(POSES) - b(POSES)).max():.2e} didepth {np.abs(a(IDEPTHS) - b(IDEPTHS)).max() if len(b(IDEPTHS)) else 0:.2e}")
    assert int(a(IT)) == int(b(IT)) and int(a(NV)) == int(b(NV)), name
    assert np.isfinite(float(a(E))) and abs(float(a(E)) - float(b(E))) <= 1e-9 * abs(float(b(E))), name
    assert np.abs(a(POSES) - b(POSES)).max() <= 1e-9, name     # poses and affine brightness
    if len(b(IDEPTHS)):
        assert np.abs(a(IDEPTHS) - b(IDEPTHS)).max() <= 1e-8 * max(1.0, np.abs(b(IDEPTHS)).max()), name
    assert np.array_equal(a(STATUSES), b(STATUSES)), name   # status and candidate status of every residual
    assert int(a(N_RESIDUAL_SWEEPS)) == int(b(N_RESIDUAL_SWEEPS)), name


ELIGIBLE = ["frames1", "frames2", "frames7", "frames8", "frames9", "landmarks1", "landmarks63", "landmarks64", "landmarks65", "landmarks130",
            "empty_frame", "missing_pair", "marginal", "rejects5", "rejects6", "first_step7", "budget7", "converges", "alone7", "alone8", "repeated",
            "alternate7", "alternate8"]
INELIGIBLE = ["sharded", "deterministic", "fixed_idepths", "no_landmarks", "many_chunks"]


@pytest.mark.parametrize("name", ELIGIBLE)
def test_fused_launch_solves_like_the_two_launches(runs, name):
    _assert_same_solve(runs, name)
    # the fused launch took the place of every reduction launch of the loop, one for one (the profile counts it with the solve launches)
    assert int(runs.get("fused", name, N_SCHUR)) == 0, name
    assert int(runs.get("split", name, N_SCHUR)) > 0, name
    assert int(runs.get("fused", name, N_SOLVE)) == int(runs.get("split", name, N_SOLVE)) == int(runs.get("split", name, N_SCHUR)), name


@pytest.mark.parametrize("name", INELIGIBLE)
def test_windows_the_fused_launch_does_not_take_keep_the_two_kernels(runs, name):
    _assert_same_solve(runs, name)
    for which in ("fused", "split"):
        assert int(runs.get(which, name, N_SCHUR)) > 0, (name, which)
    assert int(runs.get("fused", name, N_SCHUR)) == int(runs.get("split", name, N_SCHUR)), name
    assert int(runs.get("fused", name, N_SOLVE)) == int(runs.get("split", name, N_SOLVE)), name


def test_cases_reach_the_paths_they_are_named_for(runs):
    """a budget of one and of seven iterations used up, a loop that ends before its budget, a loop that rejects: the same energy after five and
    after six iterations with both budgets used up (the sixth step was evaluated and thrown away), and — the direct sign — one residual sweep
    more than a solve whose last step was accepted: the closing evaluation at the reverted state (lmSolveFusedFinish, need_final_setup).  The
    rounds behind a rejected step are the ones whose incoming control block has `relin` set: the solver decides and leaves without waiting."""
    for which in ("fused", "split"):
        assert int(runs.get(which, "first_step7", IT)) == 1 and int(runs.get(which, "budget7", IT)) == 7
        assert 3 <= int(runs.get(which, "converges", IT)) < 20
        assert int(runs.get(which, "rejects5", IT)) == 5 and int(runs.get(which, "rejects6", IT)) == 6
        e5, e6 = float(runs.get(which, "rejects5", E)), float(runs.get(which, "rejects6", E))
        assert len(runs.get(which, "rejects6", STATUSES)) > 0
        for name in ("rejects5", "rejects6"):
            assert int(runs.get(which, name, N_RESIDUAL_SWEEPS)) == int(runs.get(which, "budget7", N_RESIDUAL_SWEEPS)) + 1, (which, name)
        assert abs(e6 - e5) <= 1e-9 * abs(e5)   # (two runs that sum with atomics; an accepted sixth step that does not end the loop moves the energy by more than 1e-8 of it)


def test_back_to_back_and_alternating_solves_equal_the_window_solved_alone(runs):
    """optimize_repeated(21) is three solves of seven iterations from the snapshot, enqueued without a synchronisation in between; the two
    alternating windows are solved twice each.  Every one of those solves must be the solve of the window alone ("alone7", "alone8": the
    same process, before the others)."""
    for which in ("fused", "split"):
        assert int(runs.get(which, "repeated", IT)) == 21
        alone7, alone8 = float(runs.get(which, "alone7", E)), float(runs.get(which, "alone8", E))
        assert int(runs.get(which, "alone7", IT)) == 7   # (three solves of seven make the 21)
        assert abs(float(runs.get(which, "repeated", E)) - alone7) <= 1e-9 * abs(alone7), which
        for name, alone in (("alternate7", alone7), ("alternate8", alone8)):
            assert abs(float(runs.get(which, name, E)) - alone) <= 1e-9 * abs(alone), (which, name)
            assert abs(float(runs.get(which, name, EXTRA)) - alone) <= 1e-9 * abs(alone), (which, name)


def test_fused_launch_does_the_staged_arithmetic(runs):
    """the first step of the fused launch (7 keyframes, atomics) against assembleSolveKernel on the deterministic staged system: the bound two
    backward-stable solutions of one system obey (tests/test_gpu_dense_solve.py)"""
    eps_b, _, inputs, lam = _staged_first_step(dm.make_case_window(7), True)
    for which in ("fused", "split"):
        eps_a = runs.get(which, "first_step7", EPS)
        assert np.all(np.isfinite(eps_a))
        _assert_within_perturbation_bound(eps_a, eps_b, inputs, lam, f"{which} first step against staged F=7")
