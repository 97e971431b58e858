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
* ``TreeEnsemblePredictor`` — decision-tree ensemble (gradient boosting,
  forests) with explicit node tables; exposes ``tree_params()`` so the GPU
  engine can run the fused tree HIP kernel (split decisions packed to bits
  once per row, a bitwise select and a bit-register walk per sample).
* ``RoutedTreeEnsemblePredictor`` — the same with per-node routing of
  missing values and categorical (bitset) splits: ``HistGradientBoosting*``
  and forests fitted on data with NaN.
* ``KernelMachinePredictor`` — kernel SVM / kernel ridge (rbf or polynomial
  kernel) with explicit support vectors and dual coefficients; exposes
  ``kernel_machine_params()`` so the GPU engine can run the fused
  kernel-machine HIP kernel (squared distance / dot product folded over
  coalition groups, support vectors streamed in tiles, kernel evaluation and
  the contraction with the dual coefficients on chip).
* ``MulticlassSVCPredictor`` — multi-class one-vs-one ``SVC`` / ``NuSVC``:
  the same kernel with the pair decisions turned into one-vs-rest scores or
  coupled probabilities in a per-row epilogue.
* ``TorchPredictor`` — wraps any torch ``nn.Module`` (MLP / ResNet configs);
  the GPU engine materialises synth tiles on-device and calls the module
  stream-ordered.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

__all__ = ["KernelMachinePredictor", "LinearPredictor", "MLPPredictor",
           "MulticlassSVCPredictor", "RoutedTreeEnsemblePredictor",
           "TorchPredictor",
           "TreeEnsemblePredictor", "make_predictor"]


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


class TreeEnsemblePredictor:
    """Ensemble of binary decision trees with explicit tables:
    ``act(base + scale · Σ_t value_t(leaf_t(x)))``.

    ``trees`` is a list of dicts with per-node arrays ``feature``,
    ``threshold``, ``left``, ``right`` (root = node 0; a node with
    ``left < 0`` is a leaf) and ``value``: ``(n_nodes,)`` scalar leaves, the
    tree adding into output column ``out_col[t]``, or ``(n_nodes, n_out)``
    leaf vectors. All trees of an ensemble use the same leaf form.

    The comparison rule is sklearn's: the input is rounded to float32 and
    ``float64(x32) <= threshold`` goes left. ``__call__`` is the numpy oracle
    with exactly this rule; ``tree_params()`` is the protocol hook the GPU
    engine uses to run the fused HIP kernels (``fused_predict_trees`` for
    trees of at most 64 internal nodes, ``fused_predict_trees_walk`` for
    deeper ones); ``torch_module()`` is the fp32 gather-traversal
    ``nn.Module`` used when the ensemble is outside both envelopes.

    NaN inputs are not supported: sklearn >= 1.3 routes a missing value per
    node (``missing_go_to_left``), which these tables do not carry.
    ``__call__`` raises ``ValueError`` on a NaN; the GPU paths do not look.
    ``RoutedTreeEnsemblePredictor`` carries per-node missing-value routing
    and categorical splits (``HistGradientBoosting*``, forests fitted on
    data with NaN).
    """

    _OUT = ("softmax", "sigmoid", "none")
    _INF_THRESHOLD = False      # +inf thresholds (routed ensembles only)

    def __init__(self, trees, n_features: int, n_out: int, base=None,
                 scale: float = 1.0, out_col=None, activation: str = "none"):
        if activation not in self._OUT:
            raise ValueError(f"unknown activation {activation}")
        if len(trees) < 1:
            raise ValueError("an ensemble needs at least one tree")
        if n_out < 1 or n_features < 1:
            raise ValueError("n_out and n_features must be positive")
        self.n_features = int(n_features)
        self._n_out = int(n_out)
        self.scale = float(scale)
        self.activation = activation
        self.base = (np.zeros(n_out) if base is None
                     else np.asarray(base, dtype=np.float64).reshape(-1))
        if self.base.shape[0] != n_out:
            raise ValueError("base must have n_out entries")
        self.trees = []
        vector = None
        for ti, tr in enumerate(trees):
            feat = np.asarray(tr["feature"], dtype=np.int64).reshape(-1)
            thr = np.asarray(tr["threshold"], dtype=np.float64).reshape(-1)
            left = np.asarray(tr["left"], dtype=np.int64).reshape(-1)
            right = np.asarray(tr["right"], dtype=np.int64).reshape(-1)
            val = np.asarray(tr["value"], dtype=np.float64)
            nn_ = feat.shape[0]
            if nn_ < 1 or not (thr.shape[0] == left.shape[0] == right.shape[0]
                               == val.shape[0] == nn_):
                raise ValueError(f"tree {ti}: node arrays must be equally long")
            if val.ndim not in (1, 2) or (val.ndim == 2 and val.shape[1] != n_out):
                raise ValueError(
                    f"tree {ti}: value must be (n_nodes,) or (n_nodes, n_out)")
            if vector is None:
                vector = val.ndim == 2
            elif vector != (val.ndim == 2):
                raise ValueError("all trees must use the same leaf form")
            internal = left >= 0
            if np.any(internal != (right >= 0)):
                raise ValueError(f"tree {ti}: a node has exactly one child")
            kids = np.concatenate([left[internal], right[internal]])
            if np.any(kids >= nn_) or np.any(kids == 0) or \
                    len(np.unique(kids)) != len(kids) or len(kids) != nn_ - 1:
                raise ValueError(
                    f"tree {ti}: children must form one tree rooted at node 0")
            if np.any(feat[internal] < 0) or np.any(feat[internal] >= n_features):
                raise ValueError(f"tree {ti}: split feature out of range")
            finite = np.isfinite(thr[internal])
            if self._INF_THRESHOLD:
                finite |= thr[internal] == np.inf
            if not np.all(finite):
                raise ValueError(f"tree {ti}: thresholds must be finite"
                                 + (" or +inf" if self._INF_THRESHOLD else ""))
            self.trees.append({
                "feature": np.where(internal, feat, 0), "threshold": thr,
                "left": left, "right": right, "value": val,
            })
        self.vector_leaves = bool(vector)
        if self.vector_leaves:
            if out_col is not None:
                raise ValueError("out_col does not apply to vector leaves")
            self.out_col = None
        else:
            oc = (np.zeros(len(trees), dtype=np.int64) if out_col is None
                  else np.asarray(out_col, dtype=np.int64).reshape(-1))
            if oc.shape[0] != len(trees) or np.any(oc < 0) or np.any(oc >= n_out):
                raise ValueError("out_col must name one output column per tree")
            self.out_col = oc
        self._flat = None
        self._module = None

    @property
    def n_out(self) -> int:
        return self._n_out

    @property
    def n_trees(self) -> int:
        return len(self.trees)

    def __getstate__(self):
        # the flattened tables and the torch module are caches: a pickled
        # predictor carries the trees alone and rebuilds them on demand
        state = dict(self.__dict__)
        state["_flat"] = None
        state["_module"] = None
        return state

    # ------------------------------------------------------------------ #

    def _flatten(self):
        """Concatenated node tables with absolute child indices (leaves loop
        onto themselves), the per-tree roots and the maximum depth."""
        if self._flat is None:
            feats, thrs, lefts, rights, vals, roots = [], [], [], [], [], []
            off, depth = 0, 0
            for ti, tr in enumerate(self.trees):
                nn_ = tr["feature"].shape[0]
                internal = tr["left"] >= 0
                own = np.arange(nn_) + off
                feats.append(tr["feature"])
                thrs.append(np.where(internal, tr["threshold"], 0.0))
                lefts.append(np.where(internal, tr["left"] + off, own))
                rights.append(np.where(internal, tr["right"] + off, own))
                v = tr["value"]
                if not self.vector_leaves:
                    full = np.zeros((nn_, self._n_out))
                    full[:, self.out_col[ti]] = v
                    v = full
                vals.append(np.where(internal[:, None], 0.0, v))
                roots.append(off)
                # depth by one pass down from the root
                d = np.zeros(nn_, dtype=np.int64)
                stack = [0]
                while stack:
                    i = stack.pop()
                    if internal[i]:
                        for c in (tr["left"][i], tr["right"][i]):
                            d[c] = d[i] + 1
                            stack.append(int(c))
                depth = max(depth, int(d.max()))
                off += nn_
            self._flat = {
                "feature": np.concatenate(feats), "threshold": np.concatenate(thrs),
                "left": np.concatenate(lefts), "right": np.concatenate(rights),
                "value": np.concatenate(vals), "roots": np.asarray(roots),
                "depth": depth,
            }
        return self._flat

    def raw(self, X: np.ndarray) -> np.ndarray:
        """``base + scale · Σ_t leaf`` before the activation (fp64)."""
        f = self._flatten()
        X = np.asarray(X)
        if X.ndim != 2 or X.shape[1] != self.n_features:
            raise ValueError(f"X must be (n, {self.n_features})")
        if np.isnan(X).any():
            raise ValueError(
                "TreeEnsemblePredictor does not support NaN inputs (sklearn "
                "routes missing values per node; these tables do not)")
        # sklearn's rule: round the input to float32, compare in float64
        x32 = X.astype(np.float32).astype(np.float64)
        out = np.empty((X.shape[0], self._n_out))
        step = max(1, (1 << 22) // self.n_trees)
        for lo in range(0, X.shape[0], step):
            xs = x32[lo : lo + step]
            rows = np.arange(xs.shape[0])[:, None]
            idx = np.broadcast_to(f["roots"][None, :], (xs.shape[0], self.n_trees))
            for _ in range(f["depth"]):
                go_left = xs[rows, f["feature"][idx]] <= f["threshold"][idx]
                idx = np.where(go_left, f["left"][idx], f["right"][idx])
            out[lo : lo + step] = self.base + self.scale * f["value"][idx].sum(axis=1)
        return out

    def __call__(self, X: np.ndarray) -> np.ndarray:
        z = self.raw(X)
        if self.activation == "softmax":
            return _softmax(z)
        if self.activation == "sigmoid":
            return 1.0 / (1.0 + np.exp(-z))
        return z

    # protocol hook for the fused GPU path
    def tree_params(self):
        return {
            "trees": self.trees, "n_features": self.n_features,
            "n_out": self._n_out, "base": self.base, "scale": self.scale,
            "out_col": self.out_col, "activation": self.activation,
        }

    def build_module(self, dtype=None):
        """Gather-traversal ``nn.Module``: a node-index tensor steps
        ``max_depth`` times. fp32 (default) compares float32 rows against
        thresholds rounded down to float32, which equals the float64 rule
        exactly; float64 rounds the rows to float32 and compares in float64."""
        import torch

        from .tree_module import TreeModule

        dtype = dtype or torch.float32
        return TreeModule(self._flatten(), self.base, self.scale,
                          self.activation, dtype).eval()

    def torch_module(self):
        """fp32 module with the same tables (built once)."""
        if self._module is None:
            self._module = self.build_module()
        return self._module

    # ------------------------------------------------------------------ #

    @classmethod
    def random(cls, d: int, n_out: int = 2, trees: int = 100, depth: int = 4,
               seed: int = 0, activation: str = "softmax",
               vector_leaves: bool = False, p_stop: float = 0.2):
        """Philox-seeded ensemble of non-complete trees: below the root a
        branch ends early with probability ``p_stop``. Thresholds are drawn
        for standard-normal features; leaves are scaled so that the raw score
        has a standard deviation of about 1.5."""
        rng = np.random.Generator(np.random.Philox(key=[seed, 0x7AEE5]))
        per_col = max(1.0, trees if vector_leaves else trees / n_out)
        sigma = 1.5 / np.sqrt(per_col)
        out = []
        for _ in range(trees):
            feat, thr, left, right, val = [], [], [], [], []

            def grow(level):
                i = len(feat)
                feat.append(-1), thr.append(0.0), left.append(-1), right.append(-1)
                val.append(rng.normal(0.0, sigma, size=n_out) if vector_leaves
                           else rng.normal(0.0, sigma))
                if level < depth and (level == 0 or rng.uniform() >= p_stop):
                    feat[i] = int(rng.integers(d))
                    thr[i] = float(rng.normal())
                    left[i] = grow(level + 1)
                    right[i] = grow(level + 1)
                return i

            grow(0)
            out.append({"feature": feat, "threshold": thr, "left": left,
                        "right": right, "value": np.asarray(val)})
        out_col = None if vector_leaves else np.arange(trees) % n_out
        return cls(out, d, n_out, base=rng.normal(0.0, 0.1, size=n_out),
                   scale=1.0, out_col=out_col, activation=activation)

    @classmethod
    def from_sklearn(cls, est):
        """Wrap a fitted sklearn tree model: ``DecisionTree*``,
        ``RandomForest*`` / ``ExtraTrees*``, ``GradientBoostingRegressor`` and
        ``GradientBoostingClassifier(loss="log_loss")``. Raises ``TypeError``
        with the reason for anything else. The wrapped model agrees with
        the estimator on rows without NaN only (see the class docstring)."""
        name = type(est).__name__
        if not type(est).__module__.startswith("sklearn."):
            raise TypeError(f"{name} is not a sklearn estimator")
        if name.startswith("HistGradientBoosting"):
            raise TypeError(
                f"{name} is not supported: it compares in float64 on binned "
                "data and routes missing values and categories separately "
                "(use RoutedTreeEnsemblePredictor.from_sklearn)")
        from sklearn.ensemble import (ExtraTreesClassifier, ExtraTreesRegressor,
                                      GradientBoostingClassifier,
                                      GradientBoostingRegressor,
                                      RandomForestClassifier,
                                      RandomForestRegressor)
        from sklearn.tree import DecisionTreeClassifier, DecisionTreeRegressor

        if getattr(est, "n_outputs_", 1) != 1:
            raise TypeError(
                f"{name} was fitted on {est.n_outputs_} outputs; multi-output "
                "estimators are not supported")

        def table(tree, classes):
            t = tree.tree_
            v = t.value[:, 0, :]
            if classes:
                v = v / v.sum(axis=1, keepdims=True)
            else:
                v = v[:, 0]
            return {"feature": t.feature, "threshold": t.threshold,
                    "left": t.children_left, "right": t.children_right,
                    "value": v}

        d = int(est.n_features_in_)
        if isinstance(est, (DecisionTreeClassifier, RandomForestClassifier,
                            ExtraTreesClassifier)):
            members = [est] if isinstance(est, DecisionTreeClassifier) \
                else list(est.estimators_)
            return cls([table(m, True) for m in members], d, len(est.classes_),
                       scale=1.0 / len(members), activation="none")
        if isinstance(est, (DecisionTreeRegressor, RandomForestRegressor,
                            ExtraTreesRegressor)):
            members = [est] if isinstance(est, DecisionTreeRegressor) \
                else list(est.estimators_)
            return cls([table(m, False) for m in members], d, 1,
                       scale=1.0 / len(members), activation="none")
        if isinstance(est, (GradientBoostingRegressor, GradientBoostingClassifier)):
            stages = est.estimators_                      # (n_stages, K)
            k = stages.shape[1]
            if isinstance(est, GradientBoostingClassifier):
                if est.loss != "log_loss":
                    raise TypeError(
                        f"GradientBoostingClassifier(loss={est.loss!r}) is not "
                        "supported (only 'log_loss')")
                n_out = len(est.classes_)
                cols = [1 if k == 1 else j for _ in range(stages.shape[0])
                        for j in range(k)]
                act, score = "softmax", est.decision_function
            else:
                n_out, cols, act, score = 1, [0] * stages.shape[0], "none", est.predict
            trees = [table(stages[i, j], False)
                     for i in range(stages.shape[0]) for j in range(k)]
            pred = cls(trees, d, n_out, scale=float(est.learning_rate),
                       out_col=cols, activation=act)
            # the constant init, from the public API only: the score minus
            # our own tree sum, which must not depend on the row
            rng = np.random.Generator(np.random.Philox(key=[0, 0xBA5E]))
            probes = np.vstack([np.zeros(d), 10.0 * rng.normal(size=(2, d))])
            sc = np.asarray(score(probes), dtype=np.float64).reshape(3, -1)
            own = pred.raw(probes)
            resid = sc - (own[:, 1:2] if (k == 1 and n_out == 2) else own)
            if np.abs(resid - resid[0]).max() > 1e-9 * (1.0 + np.abs(sc).max()):
                raise TypeError(
                    f"{name} has a non-constant init estimator; only a "
                    "constant initial score can be folded into the ensemble")
            if k == 1 and n_out == 2:
                pred.base = np.array([0.0, float(resid[0, 0])])
            else:
                pred.base = resid[0].copy()
            return pred
        raise TypeError(
            f"{name} is not a supported tree model (DecisionTree*, "
            "RandomForest*, ExtraTrees*, GradientBoostingRegressor, "
            "GradientBoostingClassifier with log_loss)")


class RoutedTreeEnsemblePredictor(TreeEnsemblePredictor):
    """``TreeEnsemblePredictor`` with per-node routing of missing values and
    categorical splits (sklearn's ``HistGradientBoosting*``, and trees and
    forests fitted on data with NaN).

    Each tree dict may carry, next to the parent's arrays, ``missing_left``
    ``(n_nodes,)`` bool and ``cat_row`` ``(n_nodes,)`` int: -1 marks a numeric
    split, any other value a row of ``cat_left`` ``(C, 8)`` uint32, a bitset
    of 256 bits in which bit c set means "category code c goes left".
    ``categories`` optionally maps a feature to the sorted array of its known
    raw category values.

    Encoding, once per row (``encode``): a feature listed in ``categories``
    is replaced by the index of its float32-rounded value in that array, or
    NaN when the value is absent or NaN; every other feature is rounded to
    float32. Known category values must be exactly representable in float32,
    so that the lookup on float32 device rows agrees.

    At a node, for the encoded value v:

    * numeric: NaN routes by ``missing_left``; otherwise ``float64(v) <=
      threshold`` goes left. The threshold is finite or ``+inf`` ("every
      non-missing value goes left").
    * categorical: NaN, ``v < 0`` and ``v >= 256`` route by ``missing_left``;
      otherwise ``c = trunc(v)`` goes left iff bit c of the node's bitset is
      set. sklearn casts the value to ``uint8`` without a range check, which
      is undefined for ``v >= 256``; routing it as missing is this class's
      defined behaviour.

    sklearn's three-way rule (left set / known set / unknown treated as
    missing) is folded into the bitset at import:
    ``cat_left = raw_left | (missing_left ? ~known : 0)``.

    ``__call__`` is the numpy oracle with exactly this rule; NaN is a legal
    input. ``tree_params()`` adds a ``"routing"`` entry, which makes the GPU
    engine use the routed forms of both fused kernels.
    """

    _INF_THRESHOLD = True
    CAT_CODES = 256

    def __init__(self, trees, n_features: int, n_out: int, base=None,
                 scale: float = 1.0, out_col=None, activation: str = "none",
                 cat_left=None, categories=None):
        super().__init__(trees, n_features, n_out, base=base, scale=scale,
                         out_col=out_col, activation=activation)
        cl = (np.zeros((0, 8), dtype=np.uint32) if cat_left is None
              else np.asarray(cat_left))
        if cl.ndim != 2 or cl.shape[1] != 8 or cl.dtype != np.uint32:
            raise ValueError(
                "cat_left must be a (C, 8) uint32 array: 256 bits per "
                "categorical node")
        self.cat_left = cl.copy()
        for ti, (tr, own) in enumerate(zip(trees, self.trees)):
            nn_ = own["left"].shape[0]
            internal = own["left"] >= 0
            ml = np.asarray(tr.get("missing_left", np.zeros(nn_, dtype=bool)))
            cr = np.asarray(tr.get("cat_row", np.full(nn_, -1)))
            ml, cr = ml.reshape(-1), cr.reshape(-1).astype(np.int64)
            if ml.shape[0] != nn_ or cr.shape[0] != nn_:
                raise ValueError(
                    f"tree {ti}: missing_left and cat_row must have one "
                    "entry per node")
            cr = np.where(internal, cr, -1)
            if np.any(cr < -1) or np.any(cr >= cl.shape[0]):
                raise ValueError(
                    f"tree {ti}: cat_row must be -1 or a row of cat_left "
                    f"({cl.shape[0]} rows)")
            own["missing_left"] = ml.astype(bool) & internal
            own["cat_row"] = cr
            # a categorical split has no threshold
            own["threshold"] = np.where(cr >= 0, 0.0, own["threshold"])
        self.categories = {}
        for f, c in sorted((categories or {}).items()):
            f = int(f)
            c = np.asarray(c, dtype=np.float64).reshape(-1)
            if not 0 <= f < n_features:
                raise ValueError(f"categories: feature {f} out of range")
            if c.size < 1 or not np.all(np.isfinite(c)) \
                    or np.any(np.diff(c) <= 0):
                raise ValueError(
                    f"categories[{f}] must be finite, sorted and distinct")
            with np.errstate(over="ignore"):
                exact = c.astype(np.float32).astype(np.float64) == c
            if not np.all(exact):
                raise ValueError(
                    f"categories[{f}] must be exactly representable in "
                    "float32")
            self.categories[f] = c

    # ------------------------------------------------------------------ #

    def encode(self, X: np.ndarray) -> np.ndarray:
        """Rows as the nodes see them (fp64 holding float32 values): features
        in ``categories`` replaced by their category index or NaN, the others
        rounded to float32."""
        X = np.asarray(X)
        if X.ndim != 2 or X.shape[1] != self.n_features:
            raise ValueError(f"X must be (n, {self.n_features})")
        with np.errstate(over="ignore"):
            enc = X.astype(np.float32).astype(np.float64)
        for f, c in self.categories.items():
            v = enc[:, f]
            k = np.minimum(np.searchsorted(c, v), c.shape[0] - 1)
            enc[:, f] = np.where(c[k] == v, k.astype(np.float64), np.nan)
        return enc

    def _flatten(self):
        if self._flat is None:
            f = super()._flatten()
            f["missing_left"] = np.concatenate(
                [tr["missing_left"] for tr in self.trees])
            f["cat_row"] = np.concatenate([tr["cat_row"] for tr in self.trees])
            f["cat_left"] = self.cat_left
            f["categories"] = self.categories
        return self._flat

    def _go_left(self, f, v, idx):
        """The routing rule for encoded values ``v`` at flat nodes ``idx``."""
        ml = f["missing_left"][idx]
        cr = f["cat_row"][idx]
        nan = np.isnan(v)
        with np.errstate(invalid="ignore"):
            num = np.where(nan, ml, v <= f["threshold"][idx])
            if f["cat_left"].shape[0] == 0:
                return num
            missing = nan | (v < 0) | (v >= self.CAT_CODES)
        c = np.where(missing, 0.0, v).astype(np.int64)          # truncates
        word = f["cat_left"][np.maximum(cr, 0), c >> 5]
        bit = ((word >> (c & 31).astype(np.uint32)) & np.uint32(1)) != 0
        return np.where(cr >= 0, np.where(missing, ml, bit), num)

    def raw(self, X: np.ndarray) -> np.ndarray:
        """``base + scale · Σ_t leaf`` before the activation (fp64)."""
        f = self._flatten()
        enc = self.encode(X)
        out = np.empty((enc.shape[0], self._n_out))
        step = max(1, (1 << 22) // self.n_trees)
        for lo in range(0, enc.shape[0], step):
            xs = enc[lo : lo + step]
            rows = np.arange(xs.shape[0])[:, None]
            idx = np.broadcast_to(f["roots"][None, :], (xs.shape[0], self.n_trees))
            for _ in range(f["depth"]):
                go_left = self._go_left(f, xs[rows, f["feature"][idx]], idx)
                idx = np.where(go_left, f["left"][idx], f["right"][idx])
            out[lo : lo + step] = self.base + self.scale * f["value"][idx].sum(axis=1)
        return out

    def tree_params(self):
        params = super().tree_params()
        params["routing"] = {"cat_left": self.cat_left,
                             "categories": self.categories}
        return params

    # ------------------------------------------------------------------ #

    @classmethod
    def random(cls, d: int, n_out: int = 2, trees: int = 100, depth: int = 4,
               seed: int = 0, activation: str = "softmax",
               vector_leaves: bool = False, p_stop: float = 0.2,
               p_missing_left: float = 0.5, n_categorical: int = 0):
        """The forest ``TreeEnsemblePredictor.random`` draws for the same
        arguments, with ``missing_left`` set with probability
        ``p_missing_left`` per split and every split on one of the last
        ``n_categorical`` features turned into a categorical split with a
        random 256-bit set (those features then hold category codes)."""
        plain = TreeEnsemblePredictor.random(
            d, n_out, trees=trees, depth=depth, seed=seed,
            activation=activation, vector_leaves=vector_leaves, p_stop=p_stop)
        rng = np.random.Generator(np.random.Philox(key=[seed, 0x207ED]))
        out, sets = [], []
        for tr in plain.trees:
            nn_ = tr["left"].shape[0]
            cat = (tr["left"] >= 0) & (tr["feature"] >= d - n_categorical)
            cr = np.full(nn_, -1, dtype=np.int64)
            cr[cat] = len(sets) + np.arange(int(cat.sum()))
            for _ in range(int(cat.sum())):
                sets.append(rng.integers(0, 2**32, size=8, dtype=np.uint64)
                            .astype(np.uint32))
            out.append(dict(tr, missing_left=rng.uniform(size=nn_) < p_missing_left,
                            cat_row=cr))
        cat_left = (np.stack(sets) if sets else None)
        return cls(out, d, n_out, base=plain.base, scale=plain.scale,
                   out_col=plain.out_col, activation=activation,
                   cat_left=cat_left)

    @classmethod
    def from_sklearn(cls, est):
        """Wrap a fitted ``HistGradientBoostingClassifier`` (binary or
        multiclass), a ``HistGradientBoostingRegressor`` with an identity
        link (``squared_error``, ``absolute_error``, ``quantile``), or a
        ``DecisionTree*`` / ``RandomForest*`` / ``ExtraTrees*`` model, whose
        ``tree_.missing_go_to_left`` is carried. Raises ``TypeError`` with
        the reason for anything else."""
        name = type(est).__name__
        if not type(est).__module__.startswith("sklearn."):
            raise TypeError(f"{name} is not a sklearn estimator")
        if name in ("HistGradientBoostingClassifier",
                    "HistGradientBoostingRegressor"):
            return cls._from_hist_gradient_boosting(est)
        from sklearn.ensemble import (ExtraTreesClassifier, ExtraTreesRegressor,
                                      RandomForestClassifier,
                                      RandomForestRegressor)
        from sklearn.tree import DecisionTreeClassifier, DecisionTreeRegressor

        classes = isinstance(est, (DecisionTreeClassifier, RandomForestClassifier,
                                   ExtraTreesClassifier))
        if not classes and not isinstance(
                est, (DecisionTreeRegressor, RandomForestRegressor,
                      ExtraTreesRegressor)):
            raise TypeError(
                f"{name} has no missing-value or categorical routing to "
                "carry (supported here: HistGradientBoosting*, DecisionTree*, "
                "RandomForest*, ExtraTrees*); try "
                "TreeEnsemblePredictor.from_sklearn")
        if getattr(est, "n_outputs_", 1) != 1:
            raise TypeError(
                f"{name} was fitted on {est.n_outputs_} outputs; multi-output "
                "estimators are not supported")
        members = list(getattr(est, "estimators_", [est]))
        tables = []
        for m in members:
            t = m.tree_
            v = t.value[:, 0, :]
            v = v / v.sum(axis=1, keepdims=True) if classes else v[:, 0]
            if not hasattr(t, "missing_go_to_left"):
                raise TypeError(
                    f"{name}: tree_.missing_go_to_left is missing (sklearn "
                    ">= 1.3 is needed)")
            tables.append({"feature": t.feature, "threshold": t.threshold,
                           "left": t.children_left, "right": t.children_right,
                           "value": v,
                           "missing_left": t.missing_go_to_left != 0})
        return cls(tables, int(est.n_features_in_),
                   len(est.classes_) if classes else 1,
                   scale=1.0 / len(members), activation="none")

    @classmethod
    def _from_hist_gradient_boosting(cls, est):
        name = type(est).__name__
        classifier = name.endswith("Classifier")
        if not classifier and est.loss not in ("squared_error", "absolute_error",
                                               "quantile"):
            raise TypeError(
                f"{name}(loss={est.loss!r}) is not supported: only identity-"
                "link losses (squared_error, absolute_error, quantile)")
        try:
            stages = est._predictors
            mapper = est._bin_mapper
            pre = est._preprocessor
            known, f_idx_map = mapper.make_known_categories_bitsets()
            d = int(est.n_features_in_)
            # column j of what the trees saw is column orig[j] of the caller
            orig = np.arange(d)
            categories = {}
            if pre is not None:
                is_cat = np.asarray(est.is_categorical_, dtype=bool)
                orig = np.concatenate([np.flatnonzero(is_cat),
                                       np.flatnonzero(~is_cat)])
                enc = pre.named_transformers_["encoder"]
                for f, c in zip(np.flatnonzero(is_cat), enc.categories_):
                    c = np.asarray(c, dtype=np.float64)
                    categories[int(f)] = c[~np.isnan(c)]
            trees, sets, cols = [], [], []
            for stage in stages:
                for k, tp in enumerate(stage):
                    nd = tp.nodes
                    leaf = nd["is_leaf"] != 0
                    cat = (nd["is_categorical"] != 0) & ~leaf
                    ml = (nd["missing_go_to_left"] != 0) & ~leaf
                    fidx = np.where(leaf, 0, nd["feature_idx"]).astype(np.int64)
                    cr = np.full(nd.shape[0], -1, dtype=np.int64)
                    for i in np.flatnonzero(cat):
                        bits = np.asarray(
                            tp.raw_left_cat_bitsets[nd["bitset_idx"][i]],
                            dtype=np.uint32).copy()
                        if ml[i]:
                            # unknown categories are missing values
                            bits |= ~np.asarray(known[f_idx_map[fidx[i]]],
                                                dtype=np.uint32)
                        cr[i] = len(sets)
                        sets.append(bits)
                    trees.append({
                        "feature": orig[fidx],
                        "threshold": np.where(leaf | cat, 0.0, nd["num_threshold"]),
                        "left": np.where(leaf, -1, nd["left"].astype(np.int64)),
                        "right": np.where(leaf, -1, nd["right"].astype(np.int64)),
                        "value": nd["value"].astype(np.float64),
                        "missing_left": ml, "cat_row": cr,
                    })
                    cols.append(k)
            k = len(stages[0])
        except (AttributeError, KeyError, IndexError, ValueError) as exc:
            raise TypeError(
                f"{name}: a private attribute this import reads is missing or "
                f"different in this sklearn version ({exc})") from exc
        if classifier:
            n_out = len(est.classes_)
            if k == 1:
                cols = [1] * len(trees)
            act, score = "softmax", est.decision_function
        else:
            n_out, act, score = 1, "none", est.predict
        try:
            pred = cls(trees, d, n_out, scale=1.0, out_col=cols, activation=act,
                       cat_left=np.stack(sets) if sets else None,
                       categories=categories)
        except ValueError as exc:
            raise TypeError(f"{name}: {exc}") from exc
        # the constant baseline, from the public API only: the score minus
        # our own tree sum, which must not depend on the row
        rng = np.random.Generator(np.random.Philox(key=[0, 0xBA5E]))
        probes = np.vstack([np.zeros(d), 10.0 * rng.normal(size=(2, d))])
        probes = probes.astype(np.float32).astype(np.float64)
        sc = np.asarray(score(probes), dtype=np.float64).reshape(3, -1)
        own = pred.raw(probes)
        resid = sc - (own[:, 1:2] if (k == 1 and n_out == 2) else own)
        if np.abs(resid - resid[0]).max() > 1e-9 * (1.0 + np.abs(sc).max()):
            raise TypeError(
                f"{name}: the score minus the tree sum is not constant; the "
                "routing rule of this sklearn version differs")
        if k == 1 and n_out == 2:
            pred.base = np.array([0.0, float(resid[0, 0])])
        else:
            pred.base = resid[0].copy()
        return pred


class KernelMachinePredictor:
    """Kernel machine with explicit parameters:
    ``act(intercept + alpha · k(x, support_vectors))`` with

    * ``kernel="rbf"``:  ``k(x, v) = exp(−gamma · |x − v|²)``
    * ``kernel="poly"``: ``k(x, v) = (gamma · x·v + coef0) ** degree``

    ``support_vectors`` is ``(V, D)``, ``alpha`` ``(n_out, V)`` (dual
    coefficients), ``intercept`` ``(n_out,)``. This covers a binary
    ``SVC`` / ``NuSVC`` decision function, ``SVR`` / ``NuSVR`` and
    ``KernelRidge`` (see ``from_sklearn``).

    ``__call__`` is the fp64 numpy oracle (rbf by the explicit difference,
    chunked over rows); ``kernel_machine_params()`` is the protocol hook the
    GPU engine uses to run the fused ``fused_predict_kernelmachine`` HIP
    kernel; ``torch_module()`` is the fp32 ``nn.Module`` used when the
    machine is outside that kernel's envelope.
    """

    _OUT = ("softmax", "sigmoid", "none")
    _KERNELS = ("rbf", "poly")

    def __init__(self, support_vectors, alpha, intercept, kernel: str = "rbf",
                 gamma: float = 1.0, coef0: float = 0.0, degree: int = 3,
                 activation: str = "none"):
        if kernel not in self._KERNELS:
            raise ValueError(f"unknown kernel {kernel!r} (supported: rbf, poly)")
        if activation not in self._OUT:
            raise ValueError(f"unknown activation {activation}")
        sv = np.asarray(support_vectors, dtype=np.float64)
        if sv.ndim != 2 or sv.shape[0] < 1 or sv.shape[1] < 1:
            raise ValueError("support_vectors must be (V, D) with V, D >= 1")
        al = np.asarray(alpha, dtype=np.float64)
        if al.ndim != 2 or al.shape[0] < 1 or al.shape[1] != sv.shape[0]:
            raise ValueError("alpha must be (n_out, V)")
        ic = np.asarray(intercept, dtype=np.float64).reshape(-1)
        if ic.shape[0] != al.shape[0]:
            raise ValueError("intercept must have n_out entries")
        gamma, coef0 = float(gamma), float(coef0)
        if not np.isfinite(gamma) or gamma <= 0.0:
            raise ValueError("gamma must be positive and finite")
        if not np.isfinite(coef0):
            raise ValueError("coef0 must be finite")
        if isinstance(degree, bool) or float(degree) != int(degree) \
                or int(degree) < 1:
            raise ValueError("degree must be an integer >= 1")
        if not (np.isfinite(sv).all() and np.isfinite(al).all()
                and np.isfinite(ic).all()):
            raise ValueError(
                "support_vectors, alpha and intercept must be finite")
        self.support_vectors = sv
        self.alpha = al
        self.intercept = ic
        self.kernel = kernel
        self.gamma = gamma
        self.coef0 = coef0
        self.degree = int(degree)
        self.activation = activation
        self._module = None

    @property
    def n_out(self) -> int:
        return self.alpha.shape[0]

    @property
    def n_features(self) -> int:
        return self.support_vectors.shape[1]

    @property
    def n_sv(self) -> int:
        return self.support_vectors.shape[0]

    def __getstate__(self):
        # the torch module is a cache: a pickled predictor carries the
        # parameters alone and rebuilds it on demand
        state = dict(self.__dict__)
        state["_module"] = None
        return state

    def kernel_values(self, X: np.ndarray) -> np.ndarray:
        """``k(x, sv)`` for every row and support vector, ``(n, V)`` fp64."""
        X = np.asarray(X, dtype=np.float64)
        if self.kernel == "rbf":
            diff = X[:, None, :] - self.support_vectors[None, :, :]
            return np.exp(-self.gamma * (diff * diff).sum(axis=2))
        return (self.gamma * (X @ self.support_vectors.T)
                + self.coef0) ** self.degree

    def raw(self, X: np.ndarray) -> np.ndarray:
        """``intercept + alpha · k(x, sv)`` before the activation (fp64)."""
        X = np.asarray(X, dtype=np.float64)
        if X.ndim != 2 or X.shape[1] != self.n_features:
            raise ValueError(f"X must be (n, {self.n_features})")
        # alpha's rows, not n_out: a subclass may reduce them in its activation
        out = np.empty((X.shape[0], self.alpha.shape[0]))
        # the rbf difference tensor is (rows, V, D): bound it, not (rows, V)
        step = max(1, (1 << 22) // (self.n_sv * self.n_features))
        for lo in range(0, X.shape[0], step):
            k = self.kernel_values(X[lo : lo + step])
            out[lo : lo + step] = k @ self.alpha.T + self.intercept
        return out

    def __call__(self, X: np.ndarray) -> np.ndarray:
        z = self.raw(X)
        if self.activation == "softmax":
            return _softmax(z)
        if self.activation == "sigmoid":
            return 1.0 / (1.0 + np.exp(-z))
        return z

    # protocol hook for the fused GPU path
    def kernel_machine_params(self):
        return {
            "support_vectors": self.support_vectors, "alpha": self.alpha,
            "intercept": self.intercept, "kernel": self.kernel,
            "gamma": self.gamma, "coef0": self.coef0, "degree": self.degree,
            "activation": self.activation,
        }

    def build_module(self, dtype=None):
        """GEMM-form ``nn.Module`` with the same parameters, fp32 (default)
        or float64 (verification)."""
        import torch

        from .km_module import KernelMachineModule

        dtype = dtype or torch.float32
        return KernelMachineModule(
            self.support_vectors, self.alpha, self.intercept, self.kernel,
            self.gamma, self.coef0, self.degree, self.activation, dtype).eval()

    def torch_module(self):
        """fp32 module with the same parameters (built once)."""
        if self._module is None:
            self._module = self.build_module()
        return self._module

    # ------------------------------------------------------------------ #

    @classmethod
    def random(cls, d: int, n_out: int = 2, n_sv: int = 256,
               kernel: str = "rbf", seed: int = 0, activation: str = "softmax",
               coef0: float = 0.0, degree: int = 3):
        """Philox-seeded machine: standard-normal support vectors,
        ``gamma = 1/d``, dual coefficients scaled so that
        ``Σ_v |alpha[o, v]| = 4`` for every output (kernel values of an rbf
        machine lie in (0, 1], so the raw score stays within ±4 of the
        intercept)."""
        rng = np.random.Generator(np.random.Philox(key=[seed, 0x5F3A]))
        sv = rng.normal(size=(n_sv, d))
        alpha = rng.normal(size=(n_out, n_sv))
        alpha *= 4.0 / np.abs(alpha).sum(axis=1, keepdims=True)
        intercept = rng.normal(0.0, 0.1, size=n_out)
        return cls(sv, alpha, intercept, kernel=kernel, gamma=1.0 / d,
                   coef0=coef0, degree=degree, activation=activation)

    @classmethod
    def from_sklearn(cls, est, output: str = "decision"):
        """Wrap a fitted sklearn kernel machine with an rbf or polynomial
        kernel: a binary ``SVC`` / ``NuSVC`` (``n_out = 1``, equal to
        ``decision_function``), ``SVR`` / ``NuSVR`` and ``KernelRidge`` with
        up to 8 targets (equal to ``predict``). Raises ``TypeError`` with the
        reason for anything else. What was read from the estimator is
        checked against its public ``decision_function`` / ``predict`` on a
        few probe rows.

        ``output="proba"`` (``SVC(probability=True)`` only) gives
        ``n_out = 2``: the softmax over ``[0, −(probA·f − probB)]`` with ``f``
        the decision value, i.e. the closed-form Platt sigmoid
        ``P(classes_[1]) = 1 / (1 + exp(probA·f − probB))``. libsvm's own
        ``predict_proba`` runs an iterative pairwise coupling with a loose
        stopping tolerance even for two classes and differs from the closed
        form by about 3e-3; the probe check for this output is accordingly
        loose (2e-2) and only guards the sign convention."""
        if output not in ("decision", "proba"):
            raise ValueError(f"unknown output {output!r} (decision, proba)")
        name = type(est).__name__
        if not type(est).__module__.startswith("sklearn."):
            raise TypeError(f"{name} is not a sklearn estimator")
        svm_names = ("SVC", "NuSVC", "SVR", "NuSVR")
        if name not in svm_names + ("KernelRidge",):
            raise TypeError(
                f"{name} is not a supported kernel machine (SVC, NuSVC, SVR, "
                "NuSVR, KernelRidge)")
        kern = est.kernel
        if callable(kern):
            raise TypeError(f"{name} with a callable kernel is not supported")
        if kern == "linear":
            raise TypeError(
                f"{name}(kernel='linear') is a linear model: use "
                "LinearPredictor with its coef_ / intercept_")
        if kern in ("poly", "polynomial"):
            kern = "poly"
        elif kern != "rbf":
            raise TypeError(
                f"{name}(kernel={kern!r}) is not supported (rbf, poly)")

        def dense(a):
            return np.asarray(a.toarray() if hasattr(a, "toarray") else a,
                              dtype=np.float64)

        if name == "KernelRidge":
            sv = dense(est.X_fit_)
            alpha = dense(est.dual_coef_)
            alpha = alpha[None, :] if alpha.ndim == 1 else alpha.T
            if alpha.shape[0] > 8:
                raise TypeError(
                    f"KernelRidge with {alpha.shape[0]} targets is not "
                    "supported (at most 8)")
            intercept = np.zeros(alpha.shape[0])
            gamma = 1.0 / sv.shape[1] if est.gamma is None else float(est.gamma)
            score = est.predict
        else:
            if name in ("SVC", "NuSVC") and len(est.classes_) != 2:
                raise TypeError(
                    f"multi-class {name} ({len(est.classes_)} classes) is not "
                    "supported here: use MulticlassSVCPredictor.from_sklearn "
                    "(one-vs-one pair decisions with an ovr / coupling "
                    "epilogue)")
            sv = dense(est.support_vectors_)
            alpha = dense(est.dual_coef_).reshape(1, -1)
            intercept = np.asarray(est.intercept_, dtype=np.float64).reshape(1)
            gamma = float(est._gamma if isinstance(est.gamma, str)
                          else est.gamma)
            score = (est.decision_function if name in ("SVC", "NuSVC")
                     else est.predict)
        if output == "proba" and (
                name not in ("SVC", "NuSVC")
                or not getattr(est, "probability", False)
                or np.size(getattr(est, "probA_", ())) != 1):
            raise TypeError(
                "output='proba' needs a binary SVC / NuSVC fitted with "
                "probability=True")
        degree = est.degree if kern == "poly" else 3
        if kern == "poly" and (float(degree) != int(degree) or degree < 1):
            raise TypeError(
                f"{name} has degree {degree!r}; only integer degrees >= 1 "
                "are supported")
        coef0 = float(est.coef0) if kern == "poly" else 0.0
        try:
            pred = cls(sv, alpha, intercept, kernel=kern, gamma=gamma,
                       coef0=coef0, degree=int(degree), activation="none")
        except ValueError as e:
            raise TypeError(f"{name} cannot be wrapped: {e}") from None
        # verify what was read against the public API, on rows near a few
        # support vectors (far-away rows would only see underflowed kernels)
        rng = np.random.Generator(np.random.Philox(key=[0, 0x5EED]))
        pick = rng.integers(sv.shape[0], size=4)
        spread = sv.std(axis=0) + 1e-12
        probes = sv[pick] + 0.5 * spread * rng.normal(size=(4, sv.shape[1]))
        sc = np.asarray(score(probes), dtype=np.float64).reshape(4, -1)
        own = pred.raw(probes)
        if own.shape != sc.shape or \
                np.abs(own - sc).max() > 1e-9 * (1.0 + np.abs(sc).max()):
            raise TypeError(
                f"{name}: the parameters read from the estimator do not "
                "reproduce its decision_function / predict")
        if output == "decision":
            return pred
        pa, pb = float(est.probA_[0]), float(est.probB_[0])
        proba = cls(sv, np.vstack([np.zeros_like(alpha[0]), -pa * alpha[0]]),
                    np.array([0.0, -pa * intercept[0] + pb]), kernel=kern,
                    gamma=gamma, coef0=coef0, degree=int(degree),
                    activation="softmax")
        lib = np.asarray(est.predict_proba(probes), dtype=np.float64)
        if np.abs(proba(probes) - lib).max() > 2e-2:
            raise TypeError(
                f"{name}: the closed-form Platt sigmoid does not reproduce "
                "predict_proba (sign convention)")
        return proba


def _pair_index(n_classes: int):
    """libsvm pair order (0,1), (0,2), …, (K−2, K−1) as two index arrays."""
    i, j = np.triu_indices(n_classes, 1)
    return i.astype(np.int64), j.astype(np.int64)


class MulticlassSVCPredictor(KernelMachinePredictor):
    """Multi-class one-vs-one SVM (libsvm ``SVC`` / ``NuSVC``, K ≥ 3).

    The P = K(K−1)/2 pair decisions are ``f = intercept + alpha · k(x, sv)``
    with ``alpha`` ``(P, V)`` and ``intercept`` ``(P,)`` in libsvm pair order
    (0,1), (0,2), …, (K−2, K−1); row (i, j) is non-zero only on the support
    vectors of classes i and j. ``raw()`` returns these pair decisions.
    ``activation`` turns them into the output:

    * ``"none"``: the pair decisions themselves (sklearn's ``ovo`` decision
      function), ``n_out = P``;
    * ``"ovr"``: sklearn's ``_ovr_decision_function``: per pair, class j
      gets the vote if ``f < 0`` else class i; ``conf_i += f``,
      ``conf_j −= f``; output ``votes + conf / (3 (|conf| + 1))``,
      ``n_out = K``;
    * ``"coupling"``: libsvm's pairwise coupling at its fixed point. With
      ``r_ij = clip(1 / (1 + exp(prob_a[p] f_p + prob_b[p])), 1e-7, 1 − 1e-7)``
      and ``r_ji = 1 − r_ij``, ``Q_tt = Σ_{j≠t} r_jt²``,
      ``Q_tj = −r_jt r_tj``, the output minimises ``pᵀQp`` subject to
      ``Σp = 1`` (the (K+1) × (K+1) KKT system, solved in fp64),
      ``n_out = K``. libsvm stops its own iteration at eps = 0.005/K, so
      ``predict_proba`` differs from this by up to about 3e-3.

    ``__call__`` is the fp64 numpy oracle. The GPU engine runs the fused
    kernel-machine kernel with a one-vs-one epilogue for K ≤ 6 (``"none"``:
    P ≤ 8, i.e. K ≤ 4) and the torch module otherwise.
    """

    _OUT = ("none", "ovr", "coupling")

    def __init__(self, support_vectors, alpha, intercept, n_classes: int,
                 kernel: str = "rbf", gamma: float = 1.0, coef0: float = 0.0,
                 degree: int = 3, activation: str = "ovr", prob_a=None,
                 prob_b=None):
        super().__init__(support_vectors, alpha, intercept, kernel=kernel,
                         gamma=gamma, coef0=coef0, degree=degree,
                         activation=activation)
        if isinstance(n_classes, bool) or int(n_classes) != n_classes \
                or int(n_classes) < 3:
            raise ValueError("n_classes must be an integer >= 3")
        k = int(n_classes)
        n_pairs = k * (k - 1) // 2
        if self.alpha.shape[0] != n_pairs:
            raise ValueError(
                f"alpha must be (P, V) with P = K(K-1)/2 = {n_pairs} rows")
        self.n_classes = k
        if activation == "coupling":
            if prob_a is None or prob_b is None:
                raise ValueError(
                    "activation='coupling' needs prob_a and prob_b")
            pa = np.asarray(prob_a, dtype=np.float64).reshape(-1)
            pb = np.asarray(prob_b, dtype=np.float64).reshape(-1)
            if pa.shape[0] != n_pairs or pb.shape[0] != n_pairs:
                raise ValueError("prob_a and prob_b must have P entries")
            if not (np.isfinite(pa).all() and np.isfinite(pb).all()):
                raise ValueError("prob_a and prob_b must be finite")
            self.prob_a, self.prob_b = pa, pb
        else:
            self.prob_a = self.prob_b = None

    @property
    def n_raw(self) -> int:
        return self.alpha.shape[0]

    @property
    def n_out(self) -> int:
        return self.n_raw if self.activation == "none" else self.n_classes

    def ovr(self, f: np.ndarray) -> np.ndarray:
        """sklearn's ``_ovr_decision_function`` of pair decisions ``(n, P)``."""
        k = self.n_classes
        votes = np.zeros((f.shape[0], k))
        conf = np.zeros((f.shape[0], k))
        for p, (i, j) in enumerate(zip(*_pair_index(k))):
            neg = f[:, p] < 0
            votes[:, j] += neg
            votes[:, i] += ~neg
            conf[:, i] += f[:, p]
            conf[:, j] -= f[:, p]
        return votes + conf / (3.0 * (np.abs(conf) + 1.0))

    def pair_probabilities(self, f: np.ndarray) -> np.ndarray:
        """``r[n, i, j]`` (diagonal 0) from pair decisions ``(n, P)``."""
        k = self.n_classes
        i, j = _pair_index(k)
        rij = np.clip(1.0 / (1.0 + np.exp(f * self.prob_a + self.prob_b)),
                      1e-7, 1.0 - 1e-7)
        r = np.zeros((f.shape[0], k, k))
        r[:, i, j] = rij
        r[:, j, i] = 1.0 - rij
        return r

    def coupling(self, f: np.ndarray) -> np.ndarray:
        """The minimiser of ``pᵀQp`` subject to ``Σp = 1`` (fp64 KKT solve)."""
        k = self.n_classes
        r = self.pair_probabilities(f)
        q = -r.transpose(0, 2, 1) * r                 # Q_tj = -r_jt r_tj
        idx = np.arange(k)
        q[:, idx, idx] = (r * r).sum(axis=1)          # Q_tt = sum_j r_jt^2
        kkt = np.zeros((f.shape[0], k + 1, k + 1))
        kkt[:, :k, :k] = q
        kkt[:, :k, k] = 1.0
        kkt[:, k, :k] = 1.0
        rhs = np.zeros((f.shape[0], k + 1, 1))
        rhs[:, k, 0] = 1.0
        return np.linalg.solve(kkt, rhs)[:, :k, 0]

    def __call__(self, X: np.ndarray) -> np.ndarray:
        f = self.raw(X)
        if self.activation == "ovr":
            return self.ovr(f)
        if self.activation == "coupling":
            return self.coupling(f)
        return f

    def kernel_machine_params(self):
        params = super().kernel_machine_params()
        params.update(n_classes=self.n_classes, prob_a=self.prob_a,
                      prob_b=self.prob_b)
        return params

    def build_module(self, dtype=None):
        import torch

        from .km_module import KernelMachineModule

        dtype = dtype or torch.float32
        return KernelMachineModule(
            self.support_vectors, self.alpha, self.intercept, self.kernel,
            self.gamma, self.coef0, self.degree, self.activation, dtype,
            n_classes=self.n_classes, prob_a=self.prob_a,
            prob_b=self.prob_b).eval()

    # ------------------------------------------------------------------ #

    @classmethod
    def random(cls, d: int, n_classes: int = 3, n_sv: int = 256,
               kernel: str = "rbf", seed: int = 0, activation: str = "ovr",
               coef0: float = 0.0, degree: int = 3):
        """Philox-seeded machine with the libsvm structure: standard-normal
        support vectors in contiguous class blocks, ``gamma = 1/d``, pair row
        (i, j) non-zero only on the blocks of classes i and j and scaled so
        that ``Σ_v |alpha[p, v]| = 4``; ``prob_a`` in (−2, −0.5), ``prob_b``
        within ±0.1 (always drawn, used by ``"coupling"``)."""
        k = int(n_classes)
        if k < 3:
            raise ValueError("n_classes must be an integer >= 3")
        if n_sv < k:
            raise ValueError("n_sv must be at least n_classes")
        rng = np.random.Generator(np.random.Philox(key=[seed, 0x0501]))
        sv = rng.normal(size=(n_sv, d))
        cuts = np.linspace(0, n_sv, k + 1).round().astype(int)
        pi, pj = _pair_index(k)
        alpha = np.zeros((pi.shape[0], n_sv))
        dense = rng.normal(size=alpha.shape)
        for p, (i, j) in enumerate(zip(pi, pj)):
            for c in (i, j):
                alpha[p, cuts[c] : cuts[c + 1]] = dense[p, cuts[c] : cuts[c + 1]]
        alpha *= 4.0 / np.abs(alpha).sum(axis=1, keepdims=True)
        intercept = rng.normal(0.0, 0.1, size=pi.shape[0])
        prob_a = -rng.uniform(0.5, 2.0, size=pi.shape[0])
        prob_b = rng.uniform(-0.1, 0.1, size=pi.shape[0])
        return cls(sv, alpha, intercept, k, kernel=kernel, gamma=1.0 / d,
                   coef0=coef0, degree=degree, activation=activation,
                   prob_a=prob_a, prob_b=prob_b)

    @classmethod
    def from_sklearn(cls, est, output: str = "decision"):
        """Wrap a fitted multi-class ``SVC`` / ``NuSVC`` with an rbf or
        polynomial kernel. ``output`` is ``"ovo"`` (the P pair decisions),
        ``"ovr"`` (K scores), ``"decision"`` (whichever of the two
        ``est.decision_function_shape`` names) or ``"proba"`` (K coupled
        probabilities; needs ``probability=True``). Outputs follow
        ``est.classes_``. Raises ``TypeError`` with the reason for anything
        else. ``ovo`` and ``ovr`` are checked against the public
        ``decision_function`` on a few probe rows (1e-9 relative), ``proba``
        against ``predict_proba`` at a loose 2e-2: libsvm stops its coupling
        iteration early (about 3e-3 from the fixed point)."""
        if output not in ("decision", "ovo", "ovr", "proba"):
            raise ValueError(
                f"unknown output {output!r} (decision, ovo, ovr, proba)")
        name = type(est).__name__
        if not type(est).__module__.startswith("sklearn."):
            raise TypeError(f"{name} is not a sklearn estimator")
        if name not in ("SVC", "NuSVC"):
            raise TypeError(
                f"{name} is not a multi-class kernel machine (SVC, NuSVC)")
        kern = est.kernel
        if callable(kern):
            raise TypeError(f"{name} with a callable kernel is not supported")
        if kern == "linear":
            raise TypeError(
                f"{name}(kernel='linear') is a linear model: use "
                "LinearPredictor with its coef_ / intercept_")
        if kern in ("poly", "polynomial"):
            kern = "poly"
        elif kern != "rbf":
            raise TypeError(
                f"{name}(kernel={kern!r}) is not supported (rbf, poly)")
        k = len(est.classes_)
        if k < 3:
            raise TypeError(
                f"binary {name}: use KernelMachinePredictor.from_sklearn")
        if output == "proba" and (
                not getattr(est, "probability", False)
                or np.size(getattr(est, "probA_", ())) != k * (k - 1) // 2):
            raise TypeError(
                f"output='proba' needs an {name} fitted with probability=True")
        degree = est.degree if kern == "poly" else 3
        if kern == "poly" and (float(degree) != int(degree) or degree < 1):
            raise TypeError(
                f"{name} has degree {degree!r}; only integer degrees >= 1 "
                "are supported")
        coef0 = float(est.coef0) if kern == "poly" else 0.0
        gamma = float(est._gamma if isinstance(est.gamma, str) else est.gamma)

        def dense(a):
            return np.asarray(a.toarray() if hasattr(a, "toarray") else a,
                              dtype=np.float64)

        sv = dense(est.support_vectors_)
        dual = dense(est.dual_coef_)                       # (K-1, V)
        start = np.concatenate([[0], np.cumsum(est.n_support_)]).astype(int)
        pi, pj = _pair_index(k)
        alpha = np.zeros((pi.shape[0], sv.shape[0]))
        # libsvm: the coefficients of class i's vectors against class j sit
        # in row j-1 (j > i) resp. row j (j < i) of dual_coef_
        for p, (i, j) in enumerate(zip(pi, pj)):
            alpha[p, start[i] : start[i + 1]] = dual[j - 1, start[i] : start[i + 1]]
            alpha[p, start[j] : start[j + 1]] = dual[i, start[j] : start[j + 1]]
        intercept = np.asarray(est.intercept_, dtype=np.float64).reshape(-1)
        if output == "decision":
            output = est.decision_function_shape
            if output not in ("ovo", "ovr"):
                raise TypeError(
                    f"{name} has decision_function_shape {output!r}")
        act = {"ovo": "none", "ovr": "ovr", "proba": "coupling"}[output]
        extra = {}
        if act == "coupling":
            extra = dict(prob_a=np.asarray(est.probA_, dtype=np.float64),
                         prob_b=np.asarray(est.probB_, dtype=np.float64))
        try:
            pred = cls(sv, alpha, intercept, k, kernel=kern, gamma=gamma,
                       coef0=coef0, degree=int(degree), activation=act, **extra)
        except ValueError as e:
            raise TypeError(f"{name} cannot be wrapped: {e}") from None
        rng = np.random.Generator(np.random.Philox(key=[0, 0x5EED]))
        pick = rng.integers(sv.shape[0], size=4)
        spread = sv.std(axis=0) + 1e-12
        probes = sv[pick] + 0.5 * spread * rng.normal(size=(4, sv.shape[1]))
        if act == "coupling":
            lib = np.asarray(est.predict_proba(probes), dtype=np.float64)
            if np.abs(pred(probes) - lib).max() > 2e-2:
                raise TypeError(
                    f"{name}: the coupled pair probabilities do not "
                    "reproduce predict_proba")
            return pred
        # a shallow copy shares the fitted arrays; the caller's estimator
        # keeps its decision_function_shape
        import copy

        view = copy.copy(est)
        view.decision_function_shape = output
        sc = np.asarray(view.decision_function(probes), dtype=np.float64)
        own = pred(probes)
        if own.shape != sc.shape or \
                np.abs(own - sc).max() > 1e-9 * (1.0 + np.abs(sc).max()):
            raise TypeError(
                f"{name}: the parameters read from the estimator do not "
                "reproduce its decision_function")
        return pred


def make_predictor(kind: str, d: int, n_out: int = 2, seed: int = 0, **kw):
    """Registry entry point used by benchmarks and serve config."""
    if kind == "linear":
        return LinearPredictor.random(d, n_out, seed)
    if kind in ("svm", "svm_fused"):
        pred = KernelMachinePredictor.random(
            d, n_out, n_sv=kw.get("n_sv", 256), kernel=kw.get("kernel", "rbf"),
            seed=seed, activation=kw.get("activation", "softmax"),
            coef0=kw.get("coef0", 0.0), degree=kw.get("degree", 3),
        )
        if kind == "svm_fused":
            return pred
        # the same seeded machine behind the generic module path, so the
        # two predict paths are directly comparable
        return TorchPredictor(pred.build_module(), device=kw.get("device"))
    if kind in ("svm_multiclass", "svm_multiclass_fused"):
        # n_out is the class count here
        pred = MulticlassSVCPredictor.random(
            d, n_out, n_sv=kw.get("n_sv", 256), kernel=kw.get("kernel", "rbf"),
            seed=seed, activation=kw.get("activation", "coupling"),
            coef0=kw.get("coef0", 0.0), degree=kw.get("degree", 3),
        )
        if kind == "svm_multiclass_fused":
            return pred
        return TorchPredictor(pred.build_module(), device=kw.get("device"))
    if kind in ("trees", "trees_fused"):
        pred = TreeEnsemblePredictor.random(
            d, n_out, trees=kw.get("trees", 100), depth=kw.get("depth", 4),
            seed=seed, activation=kw.get("activation", "softmax"),
            vector_leaves=kw.get("vector_leaves", False),
            p_stop=kw.get("p_stop", 0.2),
        )
        if kind == "trees_fused":
            return pred
        # the same seeded ensemble behind the generic module path, so the
        # two predict paths are directly comparable
        return TorchPredictor(pred.build_module(), device=kw.get("device"))
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
