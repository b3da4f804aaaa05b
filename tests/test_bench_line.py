"""The line bench.py prints must stay parseable by the driver: ONE compact JSON object below 4 KB carrying the contract's
fields, `roofline` and `cpu_baseline`, whatever the side legs grow to (round 5's 21 KB line left BENCH_r05.parsed null)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _full_objects():
    import glob
    for fn in sorted(glob.glob(os.path.join(ROOT, "profiles", "r0*_bench_default_run.json"))):
        try:
            obj = json.load(open(fn))
        except ValueError:
            continue
        if isinstance(obj, dict) and "metric" in obj:
            yield os.path.basename(fn), obj


CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config")


@pytest.mark.parametrize("name,full", list(_full_objects()))
def test_compact_line_of_every_committed_full_run(name, full):
    b = _bench()
    line = json.dumps(b.compact(full, "gpurun_out/bench_full.json"), separators=(",", ":"))
    assert len(line) < 4096, (name, len(line))
    assert "\n" not in line
    back = json.loads(line)
    for k in CONTRACT:
        assert k in back, k
    assert back["value"] == pytest.approx(full["value"], rel=1e-5)
    assert back["ms_per_step"] == pytest.approx(full["ms_per_step"], rel=1e-5)
    assert "workload" in back["config"] and "model" not in back["config"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in back["roofline"], k
    assert back["roofline"]["frac"] == pytest.approx(back["roofline"]["achieved"] / back["roofline"]["peak"], rel=1e-4)
    if "cpu_baseline" in full:
        for k in ("value", "unit", "cores", "kind", "sample"):
            assert k in back["cpu_baseline"], k


def test_compact_line_stays_bounded_when_the_side_legs_grow():
    b = _bench()
    name, full = max(_full_objects(), key=lambda t: len(json.dumps(t[1])))
    fat = json.loads(json.dumps(full))
    # forty more side legs with prose, long workload strings, a long per-rank list
    for i in range(40):
        fat.setdefault("streamed_rows", {})["m%d" % (20000 + i)] = {
            "workload": "x" * 400, "fits_per_s": 1.0e6 + i, "ms_per_step": 1.0,
            "roofline": {"kernel": "k" * 300, "bound": "hbm", "achieved": 1.0, "peak": 8000.0, "unit": "GB/s", "frac": 0.1, "traffic": None}}
    fat["config"]["workload"] = "w" * 2000
    fat["value_definition"] = "v" * 2000
    line = json.dumps(b.compact(fat, "gpurun_out/bench_full.json"), separators=(",", ":"))
    assert len(line) < 4096
    back = json.loads(line)
    for k in CONTRACT + ("roofline",):
        assert k in back
    if "cpu_baseline" in fat:
        assert "cpu_baseline" in back


def test_emit_writes_the_full_object_beside_the_line(tmp_path, monkeypatch):
    b = _bench()
    name, full = next(iter(_full_objects()))
    monkeypatch.setattr(b, "ROOT", str(tmp_path))
    line = b.emit(full)
    assert len(line) < 4096
    back = json.loads(line)
    side = json.load(open(os.path.join(str(tmp_path), back["extra_file"])))
    assert side["value"] == full["value"]
    assert json.load(open(os.path.join(str(tmp_path), "bench_full.json")))["metric"] == full["metric"]


def test_dump_outputs_writes_float_arrays_and_a_seeded_sample_above_the_limit(tmp_path, monkeypatch):
    from varpro_amd.batch import REPORT_DTYPE
    b = _bench()
    B = 1000
    rng = np.random.default_rng(1)
    alpha = rng.uniform(0.5, 8.0, (B, 2))
    rep = np.zeros(B, dtype=REPORT_DTYPE)
    rep["termination"] = rng.integers(-2, 5, B)
    rep["n_evals"] = rng.integers(1, 300, B)
    rep["objective"] = rng.random(B)
    summary = np.array([rep["objective"].sum(), 700.0, 300.0, rep["n_evals"].sum()])
    names = ("alpha", "termination", "n_evals", "objective", "summary")

    b.dump_outputs(str(tmp_path / "all"), alpha, rep, summary)
    got = {k: np.load(str(tmp_path / "all" / (k + ".npy"))) for k in names}
    assert sorted(os.listdir(str(tmp_path / "all"))) == sorted(k + ".npy" for k in names)
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["alpha"], alpha) and np.array_equal(got["summary"], summary)
    for k in ("termination", "n_evals", "objective"):
        assert np.array_equal(got[k], rep[k])

    # above the size limit: the same fixed sample of problems on every call, the whole dump within the limit
    monkeypatch.setattr(b, "DUMP_LIMIT_BYTES", 16 << 10)
    b.dump_outputs(str(tmp_path / "a"), alpha, rep, summary)
    b.dump_outputs(str(tmp_path / "b"), alpha, rep, summary)
    total = sum(os.path.getsize(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a")))
    assert total <= 16 << 10
    idx = np.load(str(tmp_path / "a" / "problem_index.npy"))
    rows = idx.astype(np.int64)
    assert 0 < rows.size < B and np.array_equal(rows, idx) and np.all(np.diff(rows) > 0)
    for k in names + ("problem_index",):
        assert np.array_equal(np.load(str(tmp_path / "a" / (k + ".npy"))), np.load(str(tmp_path / "b" / (k + ".npy"))))
    assert np.array_equal(np.load(str(tmp_path / "a" / "alpha.npy")), alpha[rows])
    assert np.array_equal(np.load(str(tmp_path / "a" / "objective.npy")), rep["objective"][rows])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    import varpro_amd as vp
    from varpro_amd import synth
    B, steps = 4096, 3
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", str(B), "--steps", str(steps), "--warmup", "1",
           "--dump-outputs", str(tmp_path)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    out = json.loads(lines[0])
    for k in CONTRACT:
        assert k in out, k
    assert out["steps"] == steps and out["warmup"] == 1 and out["unit"] == "fits/s" and out["dtype"] == "f64"
    assert abs(out["value"] - B / (out["ms_per_step"] * 1e-3)) <= 1e-6 * out["value"]
    # a plain run measures the headline alone: the rest is --full's
    for k in ("roofline", "roofline_fit", "cpu_baseline", "parity_census", "side", "extra_file"):
        assert k not in out, k
    assert "one_batch_at_a_time" not in out["config"]

    # the last timed step (k = 2) ran on handle 0: problems 0 .. B-1 of the synthetic set
    d = synth.double_exp_batch(B, m=1024, noise=1e-3)
    bp = vp.BatchProblem(vp.multi_exponential_model(d["x"], d["tau_guess"][0]), d["Y"], x=d["x"])
    alpha, _c, rep = bp.fit(d["tau_guess"])
    bp.close()
    got = {k: np.load(str(tmp_path / (k + ".npy"))) for k in ("alpha", "termination", "n_evals", "objective", "summary")}
    assert got["alpha"].shape == (B, 2) and all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["termination"], rep["termination"]) and np.array_equal(got["n_evals"], rep["n_evals"])
    ok = rep["termination"] > 0
    assert np.allclose(got["alpha"][ok], alpha[ok], rtol=1e-9, atol=0)
    assert np.allclose(got["objective"], rep["objective"], rtol=1e-9, atol=0, equal_nan=True)
    cfg = out["config"]
    assert got["summary"][1] == cfg["fits_successful"] == ok.sum() and got["summary"][2] == cfg["fits_failed"]
    assert abs(got["summary"][3] - cfg["mean_evaluations_per_fit"] * B) < 0.5
    assert got["summary"][0] == pytest.approx(cfg["sum_cost"], rel=1e-12)
