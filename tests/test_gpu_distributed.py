"""N > 1 path of the HIP library on a real GPU: two processes share cuda:0, each owns one landmark shard of the window and
the C-ABI's all-reduce callback runs torch.distributed over gloo on the device buffers (the bench uses the same callback
over nccl = RCCL with one GPU per rank; two ranks cannot share one device under RCCL).  The sharded solve must reproduce
the single-window solve: the K x K sums, energies and the global outlier threshold are all combined across ranks."""
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, lm_mode, out):
    import torch
    import torch.distributed as dist
    from dsopp_amd import capi, distributed, synthetic as syn
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        win = syn.make_window(num_frames=4, num_points=400, width=320, height=240, seed=5)
        ref = None
        if rank == 0:
            g0 = capi.HipWindow(capi.default_pba_options())
            syn.load_window(g0, win)
            g0.set_lm_mode(lm_mode)
            ref = (g0.solve(), [g0.get_pose(f.frame_id) for f in win.frames])
            g0.close()
        distributed.shard_window(win, rank, world)
        stream = torch.cuda.Stream()
        g = capi.HipWindow(capi.default_pba_options(), device=0, stream=stream.cuda_stream)
        syn.load_window(g, win)
        g.set_allreduce(distributed.make_device_allreduce(dist, torch, stream, 0), rank, world)
        g.set_lm_mode(lm_mode)
        res = g.solve()
        poses = [g.get_pose(f.frame_id) for f in win.frames]
        # every rank must hold the same frame states
        flat = np.concatenate([np.concatenate([T, ab]) for T, ab in poses])
        summed = distributed.allreduce_numpy(dist, torch, flat)
        same = np.abs(summed - world * flat).max() <= 1e-12
        if rank == 0:
            (e0, it0, nv0), poses0 = ref
            e, it, nv = res
            ok = same and it == it0 and nv == nv0 and abs(e - e0) <= 1e-7 * abs(e0)
            for (T, ab), (T0, ab0) in zip(poses, poses0):
                ok = ok and np.abs(T - T0).max() <= 1e-7 and np.abs(ab - ab0).max() <= 1e-7
            out.put((bool(ok), float(e), float(e0), int(it), int(it0), int(nv), int(nv0)))
        g.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("lm_mode", [0, 1])
def test_sharded_solve_matches_single_window(lm_mode):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, lm_mode, out)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    res = out.get(timeout=5)
    assert res[0] is True, res


def _run_bench(extra, env_extra=None, timeout=900):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, **(env_extra or {}))
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    return subprocess.run([sys.executable, os.path.join(root, "bench.py")] + extra, cwd=root, env=env, capture_output=True, text=True, timeout=timeout)


def _full_result():
    """everything the run measured beside the compact stdout headline: bench.py --full writes it to bench_extras.json at the repo root"""
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "bench_extras.json")) as fh:
        return json.load(fh)


def test_bench_script_runs_with_two_ranks():
    """bench.py's own N > 1 path end to end, started the way the driver starts it when no launcher is involved
    (`python bench.py --gpus 2`: the script spawns its ranks through torch.distributed.run): sharding, collective, MAX-over-ranks
    block timing, rank-0 JSON line.  Two ranks share this one GPU over gloo (DSOPP_BENCH_SINGLE_DEVICE=1); on a multi-GPU node the
    same script runs one rank per GPU with the library's native ncclAllReduce.
    The N > 1 headline is STRONG scaling on BASELINE.json configs[3] (7 KF / 20 000 points in total, sharded) with the same window's
    single-GPU rate measured by rank 0 alone beside it (--full)."""
    import json
    out = _run_bench(["--gpus", "2", "--steps", "28", "--warmup", "7", "--full", "--no-extras", "--no-cpu"], {"DSOPP_BENCH_SINGLE_DEVICE": "1"})
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    assert len(lines[0]) < 4096   # the driver keeps an 8 KB tail of stdout: the headline alone goes there (round 5's 23 KB line was not parsed)
    d = json.loads(lines[0])
    full = _full_result()
    assert full["value"] == d["value"] and full["config"]["name"] == d["config"]["name"]
    assert d["n_gpus"] == 2 and d["steps"] == 28 and d["scaling"] == "strong" and d["value"] > 0
    assert d["config"]["name"] == "c3" and d["config"]["total_points"] == 20000 and d["config"]["points_per_gpu"] == 10000
    assert "roofline" in d and d["config"]["ranks"] == 2
    assert d["timing"]["blocks"] >= 1 and abs(d["value"] - 28 / (d["timing"]["block_ms_median"] * 1e-3)) <= 1e-6 * d["value"]
    assert d["same_workload_1gpu"] > 0 and abs(d["speedup"] - d["value"] / d["same_workload_1gpu"]) <= 1e-9 * d["speedup"]
    assert full["same_workload_1gpu"]["value"] == d["same_workload_1gpu"]
    # row g-1 beside it: rank 0 started ONE more process that drives "all devices" (here device 0 twice, in-process reducer) through
    # the single-process window group; its sharded solve must agree with the single-window solve it ran next to it
    wg = full["window_group"]
    assert "error" not in wg, wg
    assert wg["devices"] == [0, 0] and wg["transport"].startswith("local") and wg["value"] > 0 and wg["same_workload_1gpu"] > 0
    assert wg["iterations"][0] == wg["iterations"][1] and wg["valid_residuals"][0] == wg["valid_residuals"][1]
    assert wg["max_pose_difference_vs_single_window"] <= 1e-7 and wg["relative_energy_difference"] <= 1e-7


def test_bench_weak_scaling_workload_two_ranks():
    """--workload c1: the N = 1 headline's window (2000 points) on EVERY rank, value = ranks x iterations / time"""
    import json
    out = _run_bench(["--gpus", "2", "--steps", "28", "--warmup", "7", "--workload", "c1", "--no-extras", "--no-cpu", "--no-group"],
                     {"DSOPP_BENCH_SINGLE_DEVICE": "1"})
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    assert d["scaling"] == "weak" and d["config"]["total_points"] == 4000 and d["config"]["ranks"] == 2 and "speedup" not in d
    assert abs(d["value"] - 2 * 28 / (d["timing"]["block_ms_median"] * 1e-3)) <= 1e-6 * d["value"]


def test_bench_strong_scaling_workload_two_ranks():
    """--workload c4: the dense configuration (12 KF / 50 000 points in total) sharded; value counts whole-window iterations; --full adds
    the same window's single-GPU rate and the speedup"""
    import json
    out = _run_bench(["--gpus", "2", "--steps", "14", "--warmup", "7", "--workload", "c4", "--full", "--no-extras", "--no-cpu", "--no-group"],
                     {"DSOPP_BENCH_SINGLE_DEVICE": "1"})
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    assert d["scaling"] == "strong" and d["config"]["total_points"] == 50000 and d["config"]["points_per_gpu"] == 25000 and d["config"]["frames"] == 12
    assert abs(d["value"] - 14 / (d["timing"]["block_ms_median"] * 1e-3)) <= 1e-6 * d["value"] and d["speedup"] > 0


def test_bench_refuses_more_ranks_than_gpus():
    """`python bench.py --gpus N` on a node with fewer GPUs must fail loudly — never print a line for a smaller job"""
    import torch
    n = torch.cuda.device_count()
    out = _run_bench(["--gpus", str(n + 1), "--steps", "7", "--no-extras", "--no-cpu"], timeout=300)
    assert out.returncode != 0
    assert not [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert "GPU" in (out.stderr + out.stdout)


def test_native_communicator_single_rank():
    """dsopp_hip_comm (lazy dlopen of librccl, ncclCommInitRank, ncclAllReduce on the window's stream) with one rank: the
    sharded code path (accumulate -> one collective -> decide -> solve) must reproduce the plain solve.  Multi-rank RCCL
    needs one GPU per rank and is exercised by the driver's scaling run."""
    import torch
    from dsopp_amd import capi, synthetic as syn
    win = syn.make_window(num_frames=4, num_points=400, width=320, height=240, seed=5)
    g0 = capi.HipWindow(capi.default_pba_options())
    syn.load_window(g0, win)
    ref = (g0.solve(), [g0.get_pose(f.frame_id) for f in win.frames])
    g0.close()
    comm = capi.Comm(0, 1, 0, lambda raw: raw)
    # the collective itself: sum over one rank leaves the buffer unchanged, and is ordered on the given stream
    t = torch.arange(1000, dtype=torch.float64, device="cuda")
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    comm.allreduce(t.data_ptr(), t.numel(), st.cuda_stream)
    st.synchronize()
    assert torch.equal(t.cpu(), torch.arange(1000, dtype=torch.float64))
    for lm_mode, deterministic in ((0, False), (1, False), (0, True)):   # (deterministic: the two-stage build under the collective)
        g = capi.HipWindow(capi.default_pba_options())
        syn.load_window(g, win)
        g.set_comm(comm)
        g.set_lm_mode(lm_mode)
        g.set_deterministic(deterministic)
        e, it, nv = g.solve()
        (e0, it0, nv0), poses0 = ref
        assert (it, nv) == (it0, nv0) and abs(e - e0) <= 1e-7 * abs(e0)
        for f, (T0, ab0) in zip(win.frames, poses0):
            T, ab = g.get_pose(f.frame_id)
            assert np.abs(T - T0).max() <= 1e-7 and np.abs(ab - ab0).max() <= 1e-7
        g.set_comm(None)
        g.close()
    comm.close()
