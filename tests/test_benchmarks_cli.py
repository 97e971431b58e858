"""Smoke tests for the benchmark CLIs (tiny sizes, CPU)."""
import json
import os
import pickle
import subprocess
import sys

import pytest

ROOT = os.path.join(os.path.dirname(__file__), "..")


def _run(args, timeout=600, env_extra=None):
    env = dict(os.environ)
    if env_extra:
        env.update(env_extra)
    return subprocess.run(
        [sys.executable] + args, cwd=ROOT, capture_output=True, text=True,
        timeout=timeout, env=env,
    )


def test_bench_json_contract(tmp_path):
    r = _run(["bench.py", "--instances", "8", "--steps", "1", "--warmup", "0",
              "--device", "cpu", "--full"])
    assert r.returncode == 0, r.stderr[-800:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    obj = json.loads(line)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config"):
        assert key in obj, key
    assert obj["n_gpus"] == 1 and obj["scaling"] == "weak"
    assert obj["config"]["global_batch"] == 8
    # a reduced instance count must NOT claim the headline metric/baseline
    assert "2560 inst" not in obj["metric"]
    assert obj["vs_baseline"] is None
    assert "max_phi_err_vs_fp64" in obj


def test_bench_dump_outputs_reproducible(tmp_path):
    """--dump-outputs writes the last timed step's shap values, and two runs
    with the same arguments see the same inputs and write the same arrays."""
    import numpy as np

    dumps = []
    for name in ("a", "b"):
        d = tmp_path / name
        r = _run(["bench.py", "--instances", "8", "--steps", "2", "--warmup",
                  "0", "--device", "cpu", "--dump-outputs", str(d)])
        assert r.returncode == 0, r.stderr[-800:]
        line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
        obj = json.loads(line)
        assert obj["steps"] == 2 and obj["ms_per_step"] > 0
        # a plain run does not run the fp64 self-check
        assert obj["max_phi_err_vs_fp64"] is None
        assert sorted(os.listdir(d)) == ["shap_values_0.npy", "shap_values_1.npy"]
        dumps.append([np.load(d / f) for f in sorted(os.listdir(d))])
    for a, b in zip(*dumps):
        assert a.dtype in (np.float32, np.float64)
        assert a.shape == (8, 12)
        assert np.isfinite(a).all() and np.abs(a).max() > 0
        assert np.array_equal(a, b)


def test_bench_dump_outputs_size_cap(tmp_path, monkeypatch):
    """Outputs above the byte budget are cut to a fixed seeded row sample,
    the same rows in every array and on every call."""
    import numpy as np

    monkeypatch.syspath_prepend(os.path.abspath(ROOT))
    import bench

    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 4096)
    rng = np.random.default_rng(3)
    out = [rng.normal(size=(1000, 12)).astype(np.float32) for _ in range(2)]
    bench.dump_outputs(out, str(tmp_path / "a"))
    bench.dump_outputs(out, str(tmp_path / "b"))
    a = [np.load(tmp_path / "a" / f"shap_values_{o}.npy") for o in range(2)]
    b = [np.load(tmp_path / "b" / f"shap_values_{o}.npy") for o in range(2)]
    assert sum(x.nbytes for x in a) <= 4096
    assert a[0].shape == a[1].shape and 1 <= a[0].shape[0] < 1000
    for o in range(2):
        assert a[o].dtype == np.float32
        assert np.array_equal(a[o], b[o])
        # sampled rows are rows of the full output, in order
        idx = [int(np.flatnonzero((out[o] == row).all(axis=1))[0]) for row in a[o]]
        assert idx == sorted(idx)
    assert [int(np.flatnonzero((out[0] == r).all(axis=1))[0]) for r in a[0]] == \
        [int(np.flatnonzero((out[1] == r).all(axis=1))[0]) for r in a[1]]


def test_pool_cli_writes_results(tmp_path):
    assets = str(tmp_path / "assets")
    results = str(tmp_path / "results")
    r = _run([
        "benchmarks/pool.py", "--workers", "2", "--batch", "4", "--nruns", "1",
        "--instances", "8", "--assets-dir", assets, "--results-dir", results,
    ])
    assert r.returncode == 0, r.stderr[-800:]
    path = os.path.join(results, "ray_workers_2_bsize_4_actorfr_1.0.pkl")
    assert os.path.exists(path)
    with open(path, "rb") as f:
        res = pickle.load(f)
    assert len(res["t_elapsed"]) == 1


def test_analysis_cli(tmp_path):
    results = str(tmp_path)
    with open(os.path.join(results, "ray_workers_4_bsize_1_actorfr_1.0.pkl"), "wb") as f:
        pickle.dump({"t_elapsed": [1.0, 1.2]}, f)
    r = _run(["benchmarks/analysis.py", "--results-dir", results])
    assert r.returncode == 0
    assert "pool" in r.stdout and "4" in r.stdout


def test_serve_cli_tiny(tmp_path):
    assets = str(tmp_path / "assets")
    results = str(tmp_path / "results")
    r = _run([
        "benchmarks/serve_explanations.py", "--instances", "6", "--nruns", "1",
        "--benchmark", "0", "--concurrency", "4", "--port", "8877",
        "--assets-dir", assets, "--results-dir", results,
    ], timeout=900)
    assert r.returncode == 0, (r.stderr[-800:], r.stdout[-300:])
    assert os.path.exists(os.path.join(results, "ray_replicas_1_maxbatch_64.pkl"))
