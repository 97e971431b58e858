"""``nn.Module`` for ``KernelMachinePredictor``.

Kept in a module of its own so that ``models.predictors`` imports without
torch, while the class still lives at import level: a built module (and a
``TorchPredictor`` around it) pickles, which is how predictors reach the
worker processes of the distributed explainer.
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn


class KernelMachineModule(nn.Module):
    """``act(intercept + alpha · k(x, sv))`` as library GEMMs, chunked over
    rows so that the ``(rows, V)`` kernel matrix stays bounded.

    The rbf distance uses the ``|x|² + |sv|² − 2 x·sv`` expansion (one GEMM
    instead of a ``(rows, V, D)`` difference tensor), taken about the mean
    support vector to keep the cancellation small, and clamped at 0. This is
    the generic-path arithmetic, not the oracle's: the numpy ``__call__`` of
    the predictor takes the explicit difference.
    """

    def __init__(self, support_vectors, alpha, intercept, kernel, gamma,
                 coef0, degree, activation, dtype=torch.float32):
        super().__init__()
        self.kernel = kernel
        self.gamma = float(gamma)
        self.coef0 = float(coef0)
        self.degree = int(degree)
        self.activation = activation
        self.dtype = dtype
        sv = np.asarray(support_vectors, dtype=np.float64)
        center = sv.mean(axis=0) if kernel == "rbf" else np.zeros(sv.shape[1])
        svc = sv - center
        self.register_buffer("center", torch.from_numpy(center).to(dtype))
        self.register_buffer("svt", torch.from_numpy(svc.T.copy()).to(dtype))
        self.register_buffer(
            "sv_sq", torch.from_numpy((svc * svc).sum(axis=1)).to(dtype))
        self.register_buffer(
            "alpha_t", torch.from_numpy(np.asarray(alpha).T.copy()).to(dtype))
        self.register_buffer(
            "intercept", torch.from_numpy(np.asarray(intercept)).to(dtype))

    def forward(self, x):
        x = x.to(self.dtype)
        n_sv = self.svt.shape[1]
        outs = []
        step = max(1, (1 << 25) // n_sv)
        for lo in range(0, x.shape[0], step):
            xs = x[lo : lo + step]
            if self.kernel == "rbf":
                xs = xs - self.center
                d2 = (xs * xs).sum(dim=1, keepdim=True) + self.sv_sq \
                    - 2.0 * (xs @ self.svt)
                k = torch.exp(-self.gamma * d2.clamp_min_(0.0))
            else:
                t = self.gamma * (xs @ self.svt) + self.coef0
                k = t
                for _ in range(self.degree - 1):
                    k = k * t
            z = k @ self.alpha_t + self.intercept
            if self.activation == "softmax":
                z = torch.softmax(z, dim=-1)
            elif self.activation == "sigmoid":
                z = torch.sigmoid(z)
            outs.append(z)
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)
