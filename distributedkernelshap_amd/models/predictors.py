"""Predictor registry.

The reference's "model" is a pickled sklearn LogisticRegression invoked via
``predict_proba`` (``benchmarks/ray_pool.py:34``, ``scripts/fit_adult_model.py:27-32``).
Here predictors are first-class objects:

* ``LinearPredictor`` — native logistic-regression path; exposes
  ``linear_params()`` so the GPU engine can run the fused masked-GEMM +
  activation + background-reduction HIP kernel without materialising the
  perturbation matrix.
* ``MLPPredictor`` — feed-forward network with explicit weights; exposes
  ``mlp_params()`` so the GPU engine can run the fused MLP HIP kernel
  (first layer folded over coalition groups, hidden activations in LDS).
* ``TorchPredictor`` — wraps any torch ``nn.Module`` (MLP / ResNet configs);
  the GPU engine materialises synth tiles on-device and calls the module
  stream-ordered.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

__all__ = ["LinearPredictor", "MLPPredictor", "TorchPredictor", "make_predictor"]


def _softmax(z: np.ndarray) -> np.ndarray:
    z = z - z.max(axis=-1, keepdims=True)
    e = np.exp(z)
    return e / e.sum(axis=-1, keepdims=True)


class LinearPredictor:
    """Multinomial logistic regression: softmax(X @ W.T + b).

    Mirrors sklearn ``LogisticRegression(multi_class='multinomial').predict_proba``
    (reference ``scripts/fit_adult_model.py:27-32``) with explicit weights.
    """

    def __init__(self, weights: np.ndarray, bias: np.ndarray, activation: str = "softmax"):
        self.weights = np.asarray(weights, dtype=np.float64)  # (n_out, D)
        self.bias = np.asarray(bias, dtype=np.float64)  # (n_out,)
        if activation not in ("softmax", "sigmoid", "none"):
            raise ValueError(f"unknown activation {activation}")
        self.activation = activation

    @property
    def n_out(self) -> int:
        return self.weights.shape[0]

    def __call__(self, X: np.ndarray) -> np.ndarray:
        z = np.asarray(X, dtype=np.float64) @ self.weights.T + self.bias
        if self.activation == "softmax":
            return _softmax(z)
        if self.activation == "sigmoid":
            return 1.0 / (1.0 + np.exp(-z))
        return z

    # protocol hook for the fused GPU path
    def linear_params(self):
        return self.weights, self.bias, self.activation

    @classmethod
    def random(cls, d: int, n_out: int = 2, seed: int = 0, scale: float = 0.5,
               activation: str = "softmax"):
        rng = np.random.Generator(np.random.Philox(key=[seed, 0x11EA7]))
        w = rng.normal(0.0, scale, size=(n_out, d))
        b = rng.normal(0.0, 0.1, size=(n_out,))
        return cls(w, b, activation)


class TorchPredictor:
    """Wraps a torch module as a numpy-callable predictor.

    The module maps (n, D) float32 -> (n, n_out) probabilities. The GPU engine
    detects this class and keeps the perturbation tiles on-device
    (``torch_module()`` / ``device`` accessors), avoiding host round-trips
    (SURVEY.md §7.3 "arbitrary-predictor path").
    """

    def __init__(self, module, device: Optional[str] = None, batch_rows: int = 1 << 16):
        import torch

        self.module = module.eval()
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.device = device
        self.module.to(device)
        self.batch_rows = batch_rows

    def torch_module(self):
        return self.module

    def __call__(self, X: np.ndarray) -> np.ndarray:
        import torch

        X = np.asarray(X, dtype=np.float32)
        outs = []
        with torch.no_grad():
            for lo in range(0, X.shape[0], self.batch_rows):
                xb = torch.from_numpy(X[lo : lo + self.batch_rows]).to(self.device)
                outs.append(self.module(xb).float().cpu().numpy())
        return np.concatenate(outs, axis=0)


class MLPPredictor:
    """Feed-forward network with explicit weights:
    ``act(W_L · hid(… hid(W_1 x + b_1) …) + b_L)``.

    ``__call__`` is a pure numpy fp64 forward pass (the CPU oracle).
    ``mlp_params()`` is the protocol hook the GPU engine uses to run the
    fused ``fused_predict_mlp`` HIP kernel (perturbation rows and hidden
    activations never leave the chip); ``torch_module()`` is the fp32
    ``nn.Sequential`` equivalent used when the network is outside that
    kernel's envelope.
    """

    _OUT = ("softmax", "sigmoid", "none")
    _HID = ("relu", "tanh", "identity")

    def __init__(self, weights, biases, activation: str = "softmax",
                 hidden_activation: str = "relu"):
        self.weights = [np.asarray(w, dtype=np.float64) for w in weights]
        self.biases = [np.asarray(b, dtype=np.float64).reshape(-1) for b in biases]
        if len(self.weights) < 1 or len(self.weights) != len(self.biases):
            raise ValueError("weights and biases must be equally long, >= 1 layer")
        prev = None
        for w, b in zip(self.weights, self.biases):
            if w.ndim != 2 or b.shape[0] != w.shape[0]:
                raise ValueError("weights[i] must be (out_i, in_i) with biases[i] (out_i,)")
            if prev is not None and w.shape[1] != prev:
                raise ValueError("layer widths do not chain")
            prev = w.shape[0]
        if activation not in self._OUT:
            raise ValueError(f"unknown activation {activation}")
        if hidden_activation not in self._HID:
            raise ValueError(f"unknown hidden activation {hidden_activation}")
        self.activation = activation
        self.hidden_activation = hidden_activation
        self._module = None

    @property
    def n_out(self) -> int:
        return self.weights[-1].shape[0]

    def __call__(self, X: np.ndarray) -> np.ndarray:
        h = np.asarray(X, dtype=np.float64)
        for w, b in zip(self.weights[:-1], self.biases[:-1]):
            h = h @ w.T + b
            if self.hidden_activation == "relu":
                h = np.maximum(h, 0.0)
            elif self.hidden_activation == "tanh":
                h = np.tanh(h)
        z = h @ self.weights[-1].T + self.biases[-1]
        if self.activation == "softmax":
            return _softmax(z)
        if self.activation == "sigmoid":
            return 1.0 / (1.0 + np.exp(-z))
        return z

    # protocol hook for the fused GPU path
    def mlp_params(self):
        return self.weights, self.biases, self.hidden_activation, self.activation

    def torch_module(self):
        """fp32 ``nn.Sequential`` with the same weights (built once)."""
        if self._module is None:
            import torch
            from torch import nn

            mods = []
            last = len(self.weights) - 1
            for i, (w, b) in enumerate(zip(self.weights, self.biases)):
                lin = nn.Linear(w.shape[1], w.shape[0])
                with torch.no_grad():
                    lin.weight.copy_(torch.from_numpy(w))
                    lin.bias.copy_(torch.from_numpy(b))
                mods.append(lin)
                if i < last:
                    if self.hidden_activation == "relu":
                        mods.append(nn.ReLU())
                    elif self.hidden_activation == "tanh":
                        mods.append(nn.Tanh())
            if self.activation == "softmax":
                mods.append(nn.Softmax(dim=-1))
            elif self.activation == "sigmoid":
                mods.append(nn.Sigmoid())
            self._module = nn.Sequential(*mods).eval()
        return self._module

    @classmethod
    def random(cls, d: int, n_out: int = 2, hidden: int = 32, layers: int = 2,
               seed: int = 0, activation: str = "softmax",
               hidden_activation: str = "relu"):
        rng = np.random.Generator(np.random.Philox(key=[seed, 0x3117]))
        weights, biases = [], []
        prev = d
        for width in [hidden] * layers + [n_out]:
            weights.append(rng.normal(0.0, 1.0 / np.sqrt(prev), size=(width, prev)))
            biases.append(rng.normal(0.0, 0.1, size=(width,)))
            prev = width
        return cls(weights, biases, activation, hidden_activation)

    @classmethod
    def from_torch(cls, module):
        """Build from an ``nn.Sequential`` of ``Linear`` / ``ReLU`` / ``Tanh``
        with an optional trailing ``Softmax`` / ``Sigmoid``."""
        from torch import nn

        if not isinstance(module, nn.Sequential):
            raise TypeError(
                f"from_torch needs an nn.Sequential, got {type(module).__name__}"
            )
        mods = list(module)
        activation = "none"
        if mods and isinstance(mods[-1], nn.Softmax):
            if mods[-1].dim not in (-1, 1):
                raise TypeError("trailing Softmax must act on the last dim")
            activation = "softmax"
            mods = mods[:-1]
        elif mods and isinstance(mods[-1], nn.Sigmoid):
            activation = "sigmoid"
            mods = mods[:-1]
        weights, biases, hidden = [], [], []
        expect_linear = True
        for mod in mods:
            if expect_linear:
                if not isinstance(mod, nn.Linear):
                    raise TypeError(
                        f"unsupported module {type(mod).__name__} where a "
                        "Linear layer is expected"
                    )
                w = mod.weight.detach().double().cpu().numpy()
                weights.append(w)
                biases.append(
                    mod.bias.detach().double().cpu().numpy()
                    if mod.bias is not None else np.zeros(w.shape[0])
                )
                expect_linear = False
            elif isinstance(mod, nn.Linear):
                # two Linear layers back to back: identity in between
                hidden.append("identity")
                w = mod.weight.detach().double().cpu().numpy()
                weights.append(w)
                biases.append(
                    mod.bias.detach().double().cpu().numpy()
                    if mod.bias is not None else np.zeros(w.shape[0])
                )
            elif isinstance(mod, nn.ReLU):
                hidden.append("relu")
                expect_linear = True
            elif isinstance(mod, nn.Tanh):
                hidden.append("tanh")
                expect_linear = True
            else:
                raise TypeError(f"unsupported module {type(mod).__name__}")
        if not weights or expect_linear:
            raise TypeError("the network must end in a Linear layer "
                            "(optionally followed by Softmax / Sigmoid)")
        if len(hidden) != len(weights) - 1 or len(set(hidden)) > 1:
            raise TypeError("hidden layers must all use the same activation")
        return cls(weights, biases, activation, hidden[0] if hidden else "relu")


def make_predictor(kind: str, d: int, n_out: int = 2, seed: int = 0, **kw):
    """Registry entry point used by benchmarks and serve config."""
    if kind == "linear":
        return LinearPredictor.random(d, n_out, seed)
    if kind == "mlp":
        import torch
        from torch import nn

        torch.manual_seed(seed)
        hidden = kw.get("hidden", 256)
        layers = kw.get("layers", 2)
        mods = []
        prev = d
        for _ in range(layers):
            mods += [nn.Linear(prev, hidden), nn.ReLU()]
            prev = hidden
        mods += [nn.Linear(prev, n_out), nn.Softmax(dim=-1)]
        return TorchPredictor(nn.Sequential(*mods), device=kw.get("device"))
    if kind == "mlp_fused":
        # the same seeded torch initialisation as "mlp", so the two predict
        # paths carry identical weights and are directly comparable
        import torch
        from torch import nn

        torch.manual_seed(seed)
        hidden = kw.get("hidden", 256)
        layers = kw.get("layers", 2)
        mods = []
        prev = d
        for _ in range(layers):
            mods += [nn.Linear(prev, hidden), nn.ReLU()]
            prev = hidden
        mods += [nn.Linear(prev, n_out), nn.Softmax(dim=-1)]
        return MLPPredictor.from_torch(nn.Sequential(*mods))
    raise ValueError(f"unknown predictor kind {kind!r}")
