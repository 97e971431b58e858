"""Gather-traversal ``nn.Module`` for ``TreeEnsemblePredictor``.

Kept in a module of its own so that ``models.predictors`` imports without
torch, while the class still lives at import level: a built module (and a
``TorchPredictor`` around it) pickles, which is how predictors reach the
worker processes of the distributed explainer.
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn


def floor_f32(thr64: np.ndarray) -> np.ndarray:
    """Largest float32 not above each float64 threshold, so that for a
    float32 ``x``: ``x <= floor32(thr)``  <=>  ``float64(x) <= thr``."""
    with np.errstate(over="ignore"):
        t32 = thr64.astype(np.float32)
    above = t32.astype(np.float64) > thr64
    t32[above] = np.nextafter(t32[above], np.float32(-np.inf))
    return t32


class TreeModule(nn.Module):
    """A node-index tensor steps ``depth`` times over concatenated node
    tables (leaves loop onto themselves). fp32 compares float32 rows against
    thresholds rounded down to float32, which equals sklearn's float64 rule
    exactly; float64 rounds the rows to float32 and compares in float64.

    Tables of a ``RoutedTreeEnsemblePredictor`` (``flat`` carries
    ``missing_left``, ``cat_row``, ``cat_left`` and ``categories``) add the
    routing buffers: rows reach the module raw, are encoded once (one
    ``searchsorted`` per feature with known categories) and every step
    applies the predictor's routing rule. Without them the forward is the
    plain threshold walk."""

    def __init__(self, flat, base, scale, activation, dtype=torch.float32):
        super().__init__()
        f64 = dtype == torch.float64
        thr = flat["threshold"] if f64 else floor_f32(flat["threshold"])
        self.f64 = f64
        self.depth = int(flat["depth"])
        self.scale = float(scale)
        self.activation = activation
        self.register_buffer("feature", torch.from_numpy(flat["feature"].copy()))
        self.register_buffer("threshold", torch.from_numpy(np.array(thr)))
        self.register_buffer("left", torch.from_numpy(flat["left"].copy()))
        self.register_buffer("right", torch.from_numpy(flat["right"].copy()))
        self.register_buffer("value", torch.from_numpy(flat["value"]).to(dtype))
        self.register_buffer("roots", torch.from_numpy(flat["roots"].copy()))
        self.register_buffer("base", torch.from_numpy(np.asarray(base)).to(dtype))
        self.routed = "missing_left" in flat
        if self.routed:
            cat_left = np.asarray(flat["cat_left"], dtype=np.int64).reshape(-1, 8)
            self.has_cat = cat_left.shape[0] > 0
            if not self.has_cat:
                cat_left = np.zeros((1, 8), dtype=np.int64)
            self.register_buffer(
                "missing_left", torch.from_numpy(flat["missing_left"].copy()))
            self.register_buffer("cat_row", torch.from_numpy(flat["cat_row"].copy()))
            self.register_buffer("cat_left", torch.from_numpy(cat_left))
            self.cat_features = sorted(flat["categories"])
            for f in self.cat_features:
                self.register_buffer(
                    f"categories_{f}",
                    torch.from_numpy(flat["categories"][f].astype(np.float32)))

    def encode(self, x):
        """float32 rows with every feature that has known categories replaced
        by its category index, or NaN when the value is not among them."""
        x = x.float()
        if not self.cat_features:
            return x
        x = x.clone()
        for f in self.cat_features:
            cats = getattr(self, f"categories_{f}")
            v = x[:, f].contiguous()
            k = torch.searchsorted(cats, v).clamp_(max=cats.shape[0] - 1)
            x[:, f] = torch.where(cats[k] == v, k.to(v.dtype),
                                  torch.full_like(v, float("nan")))
        return x

    def _go_left(self, v, idx):
        ml = self.missing_left[idx]
        nan = v != v
        go = torch.where(nan, ml, v <= self.threshold[idx])
        if not self.has_cat:
            return go
        cr = self.cat_row[idx]
        missing = nan | (v < 0) | (v >= 256)
        c = torch.where(missing, torch.zeros_like(v), v).long()   # truncates
        word = self.cat_left[cr.clamp(min=0), c >> 5]
        bit = ((word >> (c & 31)) & 1) != 0
        return torch.where(cr >= 0, torch.where(missing, ml, bit), go)

    def forward(self, x):
        x = self.encode(x) if self.routed else x.float()
        if self.f64:
            x = x.double()
        n_trees = self.roots.shape[0]
        outs = []
        step = max(1, (1 << 25) // n_trees)
        for lo in range(0, x.shape[0], step):
            xs = x[lo : lo + step]
            idx = self.roots[None, :].expand(xs.shape[0], n_trees)
            for _ in range(self.depth):
                v = torch.gather(xs, 1, self.feature[idx])
                go_left = self._go_left(v, idx) if self.routed \
                    else v <= self.threshold[idx]
                idx = torch.where(go_left, self.left[idx], self.right[idx])
            z = self.base + self.scale * self.value[idx].sum(dim=1)
            if self.activation == "softmax":
                z = torch.softmax(z, dim=-1)
            elif self.activation == "sigmoid":
                z = torch.sigmoid(z)
            outs.append(z)
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)
