"""The C++ host mirror of the reference's solver interfaces (dsopp_amd/host/dsopp_hip_solvers.hpp) compiles against the
C-ABI with plain g++ and, on a GPU box, drives a full window solve + one alignment through it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "dsopp_amd", "host", "example_solvers.cpp")
LIBDIR = os.path.join(ROOT, "dsopp_amd", "lib")


def _build(tmp_path):
    exe = str(tmp_path / "example_solvers")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", SRC, f"-L{LIBDIR}", "-ldsopp_hip", f"-Wl,-rpath,{LIBDIR}",
           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    return exe


def test_host_mirror_compiles_and_fails_loudly_without_gpu(tmp_path):
    from dsopp_amd import capi
    exe = _build(tmp_path)
    if capi.device_count() > 0:
        pytest.skip("GPU present: covered by the gpu test")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "no CPU fallback" in r.stdout


def test_native_sequence_driver_compiles_and_fails_loudly_without_gpu(tmp_path):
    """dsopp_amd/host/tick_sequence.cpp (MonocularTracker::tick over the host mirror) builds with plain g++ -Werror against the C-ABI"""
    from dsopp_amd import capi
    exe = str(tmp_path / "tick_sequence")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "dsopp_amd", "host", "tick_sequence.cpp"),
                           f"-L{LIBDIR}", "-ldsopp_hip", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", exe])
    if capi.device_count() > 0:
        pytest.skip("GPU present: tests/test_gpu_tick_sequence.py runs it")
    r = subprocess.run([exe, "/nonexistent"], capture_output=True, text=True)
    assert r.returncode == 2 and "no CPU fallback" in r.stdout


def test_reference_adapters_pass_the_lint():
    """the reference-side adapters cannot be compiled here (no Eigen / Sophus / glog / OpenCV); scripts/adapter_lint.py checks what can be
    checked without a compiler: every C-ABI call exists with the declared arity, every include resolves in the reference tree and
    every member touched on a reference object is declared in the header of its type"""
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "adapter_lint.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_host_mirror_solves_on_gpu(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr


def test_synthetic_window_landmark_orders():
    """synthetic.make_window(order=...): the same landmarks, listed randomly (default), row-major, or tile by tile (what the round-4 bench's
    `spatially_ordered_landmarks` line and profiles/r04/large_loop_tile32_* used; since round 5 the library sorts behind the C-ABI)"""
    import numpy as np
    from dsopp_amd import synthetic as syn
    a = syn.make_window(3, 300, 320, 240, seed=1)
    r = syn.make_window(3, 300, 320, 240, seed=1, order="raster")
    t = syn.make_window(3, 300, 320, 240, seed=1, order="tile32")
    for fa, fr, ft in zip(a.frames, r.frames, t.frames):
        key = lambda uv: sorted(map(tuple, uv.tolist()))
        assert key(fa.uv) == key(fr.uv) == key(ft.uv)
        assert np.all(np.diff(fr.uv[:, 1] * 10000 + fr.uv[:, 0]) > 0)                                  # row-major
        tile = (ft.uv[:, 1] // 32) * 100000 + (ft.uv[:, 0] // 32)
        assert np.all(np.diff(tile) >= 0)                                                              # tiles in raster order
        same = np.diff(tile) == 0
        assert np.all(np.diff(ft.uv[:, 1] * 10000 + ft.uv[:, 0])[same] > 0)                            # raster inside a tile
        # the per-landmark data travelled with the permutation
        ia = {tuple(uv): (d, tuple(p)) for uv, d, p in zip(fa.uv.tolist(), fa.idepth_gt, fa.patch.tolist())}
        for uv, d, p in zip(ft.uv.tolist(), ft.idepth_gt, ft.patch.tolist()):
            assert ia[tuple(uv)] == (d, tuple(p))
