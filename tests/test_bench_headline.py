"""bench.py's ONE stdout line must stay parsable by the driver (it keeps an 8 KB tail): the headline is built by make_headline() from the
full result, everything else goes to bench_extras.json.  Round 5's line had grown to 23 KB and the driver recorded `parsed: null`."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _full_line():
    # the largest line the bench ever produced (round 5, 23 KB): every extra present
    with open(os.path.join(ROOT, "profiles", "r05", "bench.json")) as fh:
        line = json.load(fh)
    line["roofline"].setdefault("frac_profile", 0.18)
    line["roofline"].setdefault("profile_source", "profiles/r05/c1_kernel_stats.csv")
    line["roofline"].setdefault("profile_commit", "c4f38bc 2026-09-30T00:17:00+00:00")
    return line


def test_headline_is_compact_and_complete():
    line = _full_line()
    assert len(json.dumps(line)) > 20000   # the fixture really is the oversized line
    head = bench.make_headline(line)
    text = json.dumps(head, separators=(",", ":"))
    assert len(text) < bench.HEADLINE_MAX_BYTES < 6000
    assert "\n" not in text
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data"):
        assert k in head, k
    assert head["config"]["workload"].startswith("C1")
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "algorithmic_bytes_per_launch", "avg_launch_us"):
        assert k in head["roofline"], k
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in head["cpu_baseline"], k
    # nothing nested beyond the three objects + the second metric
    for k, v in head.items():
        if isinstance(v, dict):
            assert k in ("config", "roofline", "cpu_baseline", "timing", "frame_tracking_ms_per_frame_1280x1024"), k
    assert set(head["frame_tracking_ms_per_frame_1280x1024"]) == {"5_levels", "4_levels"}


def test_headline_refuses_to_grow():
    line = _full_line()
    line["config"]["workload"] = "x" * 5000
    with pytest.raises(RuntimeError):
        bench.make_headline(line)


def test_emit_writes_extras_file(tmp_path, monkeypatch, capsys):
    line = _full_line()
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    head, path = bench.emit(line)
    assert head["extras_file"] == "bench_extras.json"
    with open(path) as fh:
        full = json.load(fh)
    assert "tick_sequence" in full and "roofline_large_fullres" in full
    out = capsys.readouterr()
    assert out.out == ""          # stdout belongs to the headline alone; the full result goes to stderr
    assert "tick_sequence" in out.err


def _plain_line():
    # what a run without --full puts in its line: the contract keys, config and timing, none of the measurements beside them
    keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "warmup_effective", "ms_per_step", "timed_region_s", "higher_is_better",
            "scaling", "vs_baseline", "dtype", "data", "timing", "config")
    return {k: v for k, v in _full_line().items() if k in keep}


def test_full_is_off_by_default():
    assert bench.parse_args([]).full is False
    args = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert (args.full, args.steps, args.warmup, args.dump_outputs) == (False, 20, 5, None)
    assert bench.parse_args(["--full"]).full is True


def test_plain_headline_carries_the_contract_keys_only():
    line = _plain_line()
    head = bench.make_headline(line)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert head[k] == line[k], k
    assert set(head) == {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "timed_region_s", "higher_is_better",
                         "scaling", "vs_baseline", "dtype", "data", "config", "timing"}


def test_dump_outputs_writes_npy_within_budget(tmp_path):
    """--dump-outputs: one float64 .npy per array; an oversized landmark array becomes the same seeded sample every time"""
    import numpy as np
    arrays = {"energy": np.array([1.5]), "poses": np.ones((7, 7)), "affine_brightness": np.zeros((7, 2)), "idepth": np.arange(5000.0)}
    budget = 8 * (1 + 49 + 14 + 1000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays, max_bytes=budget)
    total = 0
    for name, a in arrays.items():
        x, y = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert x.dtype == np.float64 and np.array_equal(x, y)
        total += x.nbytes
        if name != "idepth":
            assert np.array_equal(x, a)
    idp = np.load(tmp_path / "a" / "idepth.npy")
    assert idp.size == 1000 and np.all(np.diff(idp) > 0) and total <= budget
    bench.dump_outputs(str(tmp_path / "c"), arrays)
    assert np.array_equal(np.load(tmp_path / "c" / "idepth.npy"), arrays["idepth"])   # under the default budget: written whole


@pytest.mark.gpu
def test_bench_steps_and_dump_outputs(tmp_path):
    """--steps K times exactly K GN iterations, ms_per_step is that region / K, and --dump-outputs leaves the C1 window's results; a run
    without --full measures nothing beside the headline"""
    import subprocess
    import numpy as np
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "7",
                        "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 10 and d["timing"]["blocks"] == 1
    assert d["metric"].startswith("Gauss-Newton") and d["unit"] == "GN iterations/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert abs(d["value"] - 10 / d["timed_region_s"]) <= 1e-9 * d["value"]
    for k in ("roofline", "cpu_baseline", "speedup_vs_cpu_port", "frame_tracking_ms_per_frame_1280x1024", "extras_file"):
        assert k not in d, k
    assert abs(d["ms_per_step"] * 10 - d["timed_region_s"] * 1e3) <= 1e-9 * d["ms_per_step"] * 10
    e, T, ab, idp = (np.load(out / f"{n}.npy") for n in ("energy", "poses", "affine_brightness", "idepth"))
    assert e.shape == (1,) and T.shape == (7, 7) and ab.shape == (7, 2) and idp.shape == (2000,)
    for a in (e, T, ab, idp):
        assert a.dtype == np.float64 and np.all(np.isfinite(a))
    assert e[0] > 0
