"""Fused MLP predict kernel vs the torch-module path, same run, same weights.

Shape of ``bench.py --config mlp``: 256 instances, 100 background rows, 64
features (64 singleton groups), hidden 256 x 2, ``l1_reg=False``. Four paths:

  torch_fp32   make_predictor("mlp")        module_autocast off
  torch_bf16   make_predictor("mlp")        module_autocast bf16
  fused_fp32   make_predictor("mlp_fused")  predict_dtype fp32
  fused_bf16   make_predictor("mlp_fused")  predict_dtype bf16

Each path runs in a child process of its own under a time limit; the driver
stops at the first child that fails. Every step is timed by a host clock
around work that ends in a device synchronise; after ``--warmup`` steps the
median and the spread of ``--steps`` timed steps are reported. The fused paths
also print ``max_phi_err_vs_fp64`` (the first ``--selfcheck`` instances
re-explained in the fp64 device mode on identical coalition masks) and a
per-stage trace.

    python benchmarks/mlp_fused.py                 # all four paths
    python benchmarks/mlp_fused.py --path fused_bf16
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
    # name: (predictor kind, KernelConfig kwargs)
    "torch_fp32": ("mlp", {"module_autocast": "off"}),
    "torch_bf16": ("mlp", {"module_autocast": "bf16"}),
    "fused_fp32": ("mlp_fused", {"predict_dtype": "fp32"}),
    "fused_bf16": ("mlp_fused", {"predict_dtype": "bf16"}),
}


def run_path(args) -> dict:
    import numpy as np
    import torch

    from distributedkernelshap_amd.config import KernelConfig
    from distributedkernelshap_amd.core.engine import KernelShapEngine
    from distributedkernelshap_amd.models import make_predictor, make_tabular

    if not torch.cuda.is_available():
        raise SystemExit("mlp_fused.py measures on a GPU; none is visible")
    kind, kkw = PATHS[args.path]
    data = make_tabular(
        n_features=64, n_instances=args.instances,
        n_background=args.background, seed=1000,
    )
    pred = make_predictor(kind, 64, 2, seed=0, hidden=256, layers=2)
    engine = KernelShapEngine(
        pred, data.background, groups=data.groups, link="logit", seed=0,
        device="cuda", kernels=KernelConfig(**kkw),
    )
    X_in = torch.from_numpy(data.X.astype(np.float32))

    def step():
        out = engine.shap_values(X=X_in, l1_reg=False)
        torch.cuda.synchronize()
        return out

    for _ in range(args.warmup):
        step()
    times = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        out = step()
        times.append(time.perf_counter() - t0)
    med = statistics.median(times)
    res = {
        "path": args.path,
        "instances": args.instances,
        "steps": args.steps,
        "warmup": args.warmup,
        "expl_per_s_median": args.instances / med,
        "expl_per_s_min": args.instances / max(times),
        "expl_per_s_max": args.instances / min(times),
        "ms_per_step_median": med * 1e3,
        "ms_per_step_all": [round(t * 1e3, 3) for t in times],
        "mlp_fused": bool(getattr(engine._gpu, "mlp_fused", False)),
    }
    if kind == "mlp_fused":
        assert res["mlp_fused"], "fused path expected but not taken"
        k = min(args.selfcheck, args.instances)
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
                    help="run one path in this process (default: all four, "
                         "each in a child process under --timeout)")
    ap.add_argument("--instances", type=int, default=256)
    ap.add_argument("--background", type=int, default=100)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--selfcheck", type=int, default=8,
                    help="instances re-explained in fp64 for the error figure")
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
        "--steps", str(args.steps), "--warmup", str(args.warmup),
        "--selfcheck", str(args.selfcheck),
    ]
    for name in ("torch_fp32", "torch_bf16", "fused_fp32", "fused_bf16"):
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
