"""Typed configuration (the reference scattered knobs over
argparse CLIs, a ``distributed_opts`` dict and Makefile env vars — here one
dataclass tree covers all tiers, loadable from TOML/dict/CLI).
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Union

__all__ = [
    "EngineConfig",
    "DistributedConfig",
    "ServeConfig",
    "BenchConfig",
    "KernelConfig",
    "Config",
]


@dataclass
class EngineConfig:
    """Algorithm-core knobs (ride-through kwargs of the reference,
    ``explainers/kernel_shap.py:835-851``)."""

    link: str = "logit"
    seed: int = 0
    nsamples: Optional[int] = None  # None -> 2*M + 2048
    l1_reg: Union[str, int, float, None] = "auto"
    device: str = "auto"
    chunk_rows: int = 1 << 20


@dataclass
class DistributedConfig:
    """Reference DISTRIBUTED_OPTS (``explainers/kernel_shap.py:210-214``)
    plus the collective-backend tier."""

    n_workers: Optional[int] = None
    batch_size: int = 1
    actor_cpu_fraction: float = 1.0
    backend: str = "auto"  # nccl (RCCL) on GPU, gloo on CPU
    mp_context: Optional[str] = None

    def to_opts(self) -> Dict[str, Any]:
        d = {
            "n_workers": self.n_workers,
            "batch_size": self.batch_size,
            "actor_cpu_fraction": self.actor_cpu_fraction,
        }
        if self.mp_context:
            d["mp_context"] = self.mp_context
        return d


@dataclass
class ServeConfig:
    host: str = "127.0.0.1"
    port: int = 8800
    replicas: int = 1
    max_batch_size: int = 64
    max_wait_ms: float = 2.0


@dataclass
class KernelConfig:
    """HIP kernel dispatch knobs (tile sizes are compile-time; these select
    code paths)."""

    wls_mode: str = "auto"  # auto | mfma | generic | torch
    fused_predict: bool = True
    # fp32: f32 MFMA (default).  bf16x2: bf16 matrix cores with a hi+lo
    # split B operand (error ~2^-16, fp32-grade, ~6x less MFMA issue time).
    # bf16: single bf16 image (fastest, ~0.4% relative ey error).
    # fp64: full-double verification mode (linear predictors) — the
    # reference's numpy-fp64 arithmetic, used by bench.py's self-check.
    predict_dtype: str = "fp32"  # fp32 | bf16x2 | bf16 | fp64
    # matrix instruction of the packed linear predict (fp32 results either
    # way).  split: bf16 matrix cores on an exact three-piece bf16 split of
    # the fp32 operands (mask bits x pieces are exact products, fp32
    # accumulation), eligible for the sigmoid-type activations with at most
    # 12 varying groups; other shapes take the f32 MFMA silently.  auto:
    # split where eligible.  Non-finite weights or inputs are outside the
    # split path's contract: inf - inf in the split gives NaN where the f32
    # MFMA gives a saturated probability.
    packed_mma: str = "auto"  # auto | f32 | split
    synth_chunk_rows: int = 1 << 21  # ~0.5 GB synth tiles: +15% on mlp vs 2^19
    # l1_reg selection on GPU batches: True = device Gram + batched torch
    # LARS (core.lars), False = per-instance host sklearn (the CPU oracle's
    # path, kept as a cross-check)
    l1_device: bool = True
    # torch-module predictor path (mlp/resnet configs): bf16 autocast around
    # the module forward ("bf16") and channels-last weight layout for conv
    # nets — the predict-bound configs' main levers on MI355X matrix cores.
    # channels_last only applies WITH bf16 autocast: MIOpen's fp32 NCHW
    # path measured faster than NHWC (5.4 vs 3.2 expl/s on resnet), while
    # bf16 NHWC wins (14.4 vs 12.4)
    module_autocast: str = "off"  # off | bf16
    module_channels_last: bool = True


@dataclass
class BenchConfig:
    instances: int = 2560
    background: int = 100
    nruns: int = 5
    steps: int = 5
    warmup: int = 2
    batch_sizes: List[int] = field(default_factory=lambda: [1, 5, 10])
    results_dir: str = "results"
    assets_dir: str = "assets"


@dataclass
class Config:
    engine: EngineConfig = field(default_factory=EngineConfig)
    distributed: DistributedConfig = field(default_factory=DistributedConfig)
    serve: ServeConfig = field(default_factory=ServeConfig)
    kernels: KernelConfig = field(default_factory=KernelConfig)
    bench: BenchConfig = field(default_factory=BenchConfig)

    @classmethod
    def from_dict(cls, d: Dict[str, Any]) -> "Config":
        cfg = cls()
        for section, values in d.items():
            if not hasattr(cfg, section):
                raise KeyError(f"unknown config section '{section}'")
            sub = getattr(cfg, section)
            names = {f.name for f in dataclasses.fields(sub)}
            for k, v in values.items():
                if k not in names:
                    raise KeyError(f"unknown key '{section}.{k}'")
                setattr(sub, k, v)
        return cfg

    @classmethod
    def from_toml(cls, path: str) -> "Config":
        import tomli

        with open(path, "rb") as f:
            return cls.from_dict(tomli.load(f))

    def to_dict(self) -> Dict[str, Any]:
        return dataclasses.asdict(self)
