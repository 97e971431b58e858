"""Fused tree predict kernel vs the torch-module path, same run, same ensemble.

Default shape: 256 instances, 100 background rows, 64 features (64 singleton
groups), 100 trees of depth 4, default sample count, ``l1_reg=False``. Paths:

  module   make_predictor("trees")        gather-traversal module on synth rows
  fused    make_predictor("trees_fused")  fused_predict_trees, or
                                          fused_predict_trees_walk for trees
                                          of more than 64 internal nodes
  cpu      make_predictor("trees_fused")  CPU engine on ``--cpu-instances`` rows

Each path runs in a child process of its own under a time limit; the driver
stops at the first child that fails. Every step is timed by a host clock
around work that ends in a device synchronise; after ``--warmup`` steps the
median and the spread of ``--steps`` timed steps are reported. The fused path
also prints ``max_phi_err_vs_fp64`` (the first ``--selfcheck`` instances
re-explained in the fp64 device mode on identical coalition masks); both GPU
paths print a per-stage trace.

    python benchmarks/trees_fused.py                 # all three paths
    python benchmarks/trees_fused.py --path fused
    # a forest shape (about 280 internal nodes per tree): the walk kernel;
    # the module path explains fewer rows so that it ends within --timeout
    python benchmarks/trees_fused.py --depth 12 --p-stop 0.2 --module-instances 8
    # the same forest as a routed ensemble (RoutedTreeEnsemblePredictor):
    # missing_left set with --p-missing-left (0.5), the splits on the last
    # --n-categorical (8) features categorical, those columns holding
    # category codes, NaN in --p-nan (5 %) of the entries of the instances
    # and of the background
    python benchmarks/trees_fused.py --routed --depth 12 --p-stop 0.2 \
        --module-instances 8
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

PATHS = {
    # name: (predictor kind, device)
    "module": ("trees", "cuda"),
    "fused": ("trees_fused", "cuda"),
    "cpu": ("trees_fused", "cpu"),
}


def routed_problem(args, kind, data):
    """The forest of the unrouted run with routing added, and ``data``
    changed in place: category codes in the last columns, NaN sprinkled over
    the instances and the background."""
    import numpy as np

    from distributedkernelshap_amd.models import (RoutedTreeEnsemblePredictor,
                                                  TorchPredictor)

    pred = RoutedTreeEnsemblePredictor.random(
        64, 2, seed=0, trees=args.trees, depth=args.depth, p_stop=args.p_stop,
        p_missing_left=args.p_missing_left, n_categorical=args.n_categorical)
    rng = np.random.Generator(np.random.Philox(key=[1000, 0x207ED]))
    for a in (data.X, data.background):
        if args.n_categorical:
            a[:, -args.n_categorical:] = rng.integers(
                0, 256, size=(a.shape[0], args.n_categorical))
        a[rng.uniform(size=a.shape) < args.p_nan] = np.nan
    if kind == "trees_fused":
        return pred
    return TorchPredictor(pred.build_module(), device="cuda")


def run_path(args) -> dict:
    import numpy as np
    import torch

    from distributedkernelshap_amd.config import KernelConfig
    from distributedkernelshap_amd.core.engine import KernelShapEngine
    from distributedkernelshap_amd.models import make_predictor, make_tabular

    if not torch.cuda.is_available():
        raise SystemExit("trees_fused.py measures on a GPU; none is visible")
    kind, device = PATHS[args.path]
    instances = args.cpu_instances if device == "cpu" else args.instances
    if args.path == "module" and args.module_instances is not None:
        instances = args.module_instances
    data = make_tabular(
        n_features=64, n_instances=args.instances,
        n_background=args.background, seed=1000,
    )
    if args.routed:
        pred = routed_problem(args, kind, data)
    else:
        pred = make_predictor(kind, 64, 2, seed=0, trees=args.trees,
                              depth=args.depth, p_stop=args.p_stop)
    engine = KernelShapEngine(
        pred, data.background, groups=data.groups, link="logit", seed=0,
        device=device,
    )
    X_np = data.X[:instances]
    X_in = torch.from_numpy(X_np.astype(np.float32)) if device == "cuda" else X_np

    def step():
        out = engine.shap_values(X=X_in, l1_reg=False)
        if device == "cuda":
            torch.cuda.synchronize()
        return out

    warmup, steps = (0, 1) if device == "cpu" else (args.warmup, args.steps)
    for _ in range(warmup):
        step()
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        out = step()
        times.append(time.perf_counter() - t0)
    med = statistics.median(times)
    res = {
        "path": args.path,
        "instances": instances,
        "trees": args.trees,
        "depth": args.depth,
        "routed": bool(args.routed),
        "steps": steps,
        "warmup": warmup,
        "expl_per_s_median": instances / med,
        "expl_per_s_min": instances / max(times),
        "expl_per_s_max": instances / min(times),
        "ms_per_step_median": med * 1e3,
        "ms_per_step_all": [round(t * 1e3, 3) for t in times],
    }
    if device == "cpu":
        return res
    res["trees_fused"] = bool(getattr(engine._gpu, "trees_fused", False))
    res["trees_kernel"] = getattr(engine._gpu, "trees_kernel", None)
    if kind == "trees_fused":
        assert res["trees_fused"], "fused path expected but not taken"
        k = min(args.selfcheck, instances)
        eng64 = KernelShapEngine(
            pred, data.background, groups=data.groups, link="logit", seed=0,
            device="cuda", kernels=KernelConfig(predict_dtype="fp64"),
        )
        sv64 = eng64.shap_values(data.X[:k], l1_reg=False)
        sv = engine.shap_values(data.X[:k], l1_reg=False)
        res["max_phi_err_vs_fp64"] = float(
            max(np.abs(sv[o] - sv64[o]).max() for o in range(len(sv64)))
        )
        res["max_abs_phi_fp64"] = float(max(np.abs(s).max() for s in sv64))
    del out
    engine.enable_tracing(True)
    step()
    res["trace_ms"] = {
        name: round(sum(v), 3) for name, v in engine.get_trace().items()
    }
    return res


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--path", choices=sorted(PATHS), default=None,
                    help="run one path in this process (default: all three, "
                         "each in a child process under --timeout)")
    ap.add_argument("--instances", type=int, default=256)
    ap.add_argument("--background", type=int, default=100)
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--p-stop", type=float, default=0.2,
                    help="probability that a branch below the root ends early")
    ap.add_argument("--routed", action="store_true",
                    help="the same forest with missing-value and categorical "
                         "routing, NaN in the rows (RoutedTreeEnsemblePredictor)")
    ap.add_argument("--n-categorical", type=int, default=8,
                    help="--routed: the last N of the 64 features hold "
                         "category codes and split categorically")
    ap.add_argument("--p-nan", type=float, default=0.05,
                    help="--routed: share of NaN entries in the instances "
                         "and in the background")
    ap.add_argument("--p-missing-left", type=float, default=0.5,
                    help="--routed: probability of a split's missing_left flag")
    ap.add_argument("--module-instances", type=int, default=None,
                    help="instances the module path explains (default: "
                         "--instances); for deep shapes")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--selfcheck", type=int, default=8,
                    help="instances re-explained in fp64 for the error figure")
    ap.add_argument("--cpu-instances", type=int, default=2,
                    help="instances the CPU engine explains, once, for scale")
    ap.add_argument("--timeout", type=float, default=240.0,
                    help="seconds per child process")
    args = ap.parse_args()
    if args.steps < 5:
        ap.error("--steps must be at least 5 (median and spread)")

    if args.path is not None:
        print(json.dumps(run_path(args)), flush=True)
        return

    passthrough = [
        "--instances", str(args.instances), "--background", str(args.background),
        "--trees", str(args.trees), "--depth", str(args.depth),
        "--p-stop", str(args.p_stop),
        "--steps", str(args.steps), "--warmup", str(args.warmup),
        "--selfcheck", str(args.selfcheck),
        "--cpu-instances", str(args.cpu_instances),
    ]
    if args.module_instances is not None:
        passthrough += ["--module-instances", str(args.module_instances)]
    if args.routed:
        passthrough += ["--routed", "--n-categorical", str(args.n_categorical),
                        "--p-nan", str(args.p_nan),
                        "--p-missing-left", str(args.p_missing_left)]
    for name in ("module", "fused", "cpu"):
        cmd = [sys.executable, os.path.abspath(__file__), "--path", name]
        try:
            proc = subprocess.run(cmd + passthrough, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"{name}: no result within {args.timeout:.0f} s; "
                             "stopping")
        if proc.returncode != 0:
            raise SystemExit(f"{name}: exit status {proc.returncode}; stopping")


if __name__ == "__main__":
    main()
