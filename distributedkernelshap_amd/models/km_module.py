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
    rows so that the ``(rows, V)`` kernel matrix stays bounded. ``act`` is
    none / sigmoid / softmax, or the one-vs-one epilogues ``"ovr"`` and
    ``"coupling"`` of ``MulticlassSVCPredictor`` (``n_classes``, ``prob_a``,
    ``prob_b``), batched over rows in the module's dtype.

    The rbf distance uses the ``|x|² + |sv|² − 2 x·sv`` expansion (one GEMM
    instead of a ``(rows, V, D)`` difference tensor), taken about the mean
    support vector to keep the cancellation small, and clamped at 0. This is
    the generic-path arithmetic, not the oracle's: the numpy ``__call__`` of
    the predictor takes the explicit difference.
    """

    def __init__(self, support_vectors, alpha, intercept, kernel, gamma,
                 coef0, degree, activation, dtype=torch.float32,
                 n_classes=None, prob_a=None, prob_b=None):
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
        if activation in ("ovr", "coupling"):
            # one-vs-one epilogue of MulticlassSVCPredictor: libsvm pair order
            self.n_classes = int(n_classes)
            pi, pj = np.triu_indices(self.n_classes, 1)
            self.register_buffer("pair_i", torch.from_numpy(pi.astype(np.int64)))
            self.register_buffer("pair_j", torch.from_numpy(pj.astype(np.int64)))
        if activation == "coupling":
            self.register_buffer(
                "prob_a", torch.from_numpy(np.asarray(prob_a)).to(dtype))
            self.register_buffer(
                "prob_b", torch.from_numpy(np.asarray(prob_b)).to(dtype))

    def _ovr(self, f):
        """sklearn's ``_ovr_decision_function`` of pair decisions (n, P)."""
        n, k = f.shape[0], self.n_classes
        neg = (f < 0).to(f.dtype)
        votes = f.new_zeros(n, k)
        votes.index_add_(1, self.pair_j, neg)
        votes.index_add_(1, self.pair_i, 1.0 - neg)
        conf = f.new_zeros(n, k)
        conf.index_add_(1, self.pair_i, f)
        conf.index_add_(1, self.pair_j, -f)
        return votes + conf / (3.0 * (conf.abs() + 1.0))

    def _coupling(self, f):
        """Pairwise coupling at its fixed point: the KKT system
        ``[[Q, 1], [1ᵀ, 0]] [p; λ] = [0; 1]`` by LU with partial pivoting in
        the module's dtype, the algorithm (and operation order) of the fused
        kernel's epilogue. ``r_ji`` is the sigmoid of the negated argument,
        not ``1 − r_ij``."""
        n, k = f.shape[0], self.n_classes
        arg = f * self.prob_a + self.prob_b
        rij = (1.0 / (1.0 + torch.exp(arg))).clamp(1e-7, 1.0 - 1e-7)
        rji = (1.0 / (1.0 + torch.exp(-arg))).clamp(1e-7, 1.0 - 1e-7)
        m = k + 1
        a = f.new_zeros(n, m, m + 1)                  # augmented [KKT | rhs]
        a[:, self.pair_i, self.pair_j] = -rij * rji
        a[:, self.pair_j, self.pair_i] = -rij * rji
        diag = f.new_zeros(n, k)
        diag.index_add_(1, self.pair_i, rji * rji)    # Q_ii += r_ji^2
        diag.index_add_(1, self.pair_j, rij * rij)    # Q_jj += r_ij^2
        idx = torch.arange(k, device=f.device)
        a[:, idx, idx] = diag
        a[:, :k, k] = 1.0
        a[:, k, :k] = 1.0
        a[:, k, m] = 1.0
        rows = torch.arange(n, device=f.device)
        inv = f.new_zeros(n, m)
        for c in range(m):
            piv = a[:, c:, c].abs().argmax(dim=1) + c     # first maximum
            rc = a[:, c].clone()
            a[:, c] = a[rows, piv]
            a[rows, piv] = rc
            inv[:, c] = 1.0 / a[:, c, c]
            if c + 1 < m:
                mult = a[:, c + 1 :, c] * inv[:, c, None]
                a[:, c + 1 :] = a[:, c + 1 :] - mult[:, :, None] * a[:, c : c + 1]
        x = f.new_zeros(n, m)
        for c in range(m - 1, -1, -1):
            acc = a[:, c, m] - (a[:, c, c + 1 : m] * x[:, c + 1 :]).sum(dim=1)
            x[:, c] = acc * inv[:, c]
        return x[:, :k]

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
            elif self.activation == "ovr":
                z = self._ovr(z)
            elif self.activation == "coupling":
                z = self._coupling(z)
            outs.append(z)
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)
