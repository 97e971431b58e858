"""Per-family predict backends of the GPU engine: MLP (K4m), tree ensemble
(K4t / K4w) and kernel machine (K4k / K4kp).

A backend is built from ``(gpu, predictor)`` at fit time and owns what its
family needs: the fp32 torch ``module`` of the fallback path, the fp64
forward behind the per-instance totals, the packed operands of the fused
kernel, and (``predict_dtype='fp64'`` only) the unrounded fit-time constants
of the verification mode. ``GpuKernelShap.backend`` is ``None`` for linear
and plain torch-module predictors.
"""
from __future__ import annotations

import copy
import logging

import numpy as np
import torch

from . import km_pack, mlp_pack, tree_pack

# the engine's logger: one place for users to filter the fallback reasons
logger = logging.getLogger(__package__ + ".gpu_engine")


def blend_ey_f64(masks, X64, bg64, wbg64, col_to_mask_col, forward, n_out,
                 width, budget_bytes=256 << 20):
    """fp64 ey (b, S, n_out) by the explicit masked blend: row (b, s, n) is
    ``X64[b]`` where the sample's mask is on and ``bg64[n]`` elsewhere, goes
    through ``forward`` ((b, sc, N, D) -> (b, sc, N, n_out)) and is averaged
    with ``wbg64``. ``col_to_mask_col`` (D,) maps a column to its group's
    mask column, non-varying ones to the sentinel ``m``. Chunked over samples
    so that three ``width``-wide fp64 row tensors stay within
    ``budget_bytes``. Device-agnostic."""
    b, s, m = masks.shape
    n = bg64.shape[0]
    s_chunk = max(1, budget_bytes // (8 * 3 * b * n * width))
    ey = torch.empty(b, s, n_out, dtype=torch.float64, device=masks.device)
    zero_col = torch.zeros(b, 1, 1, dtype=torch.bool, device=masks.device)
    for lo in range(0, s, s_chunk):
        hi = min(lo + s_chunk, s)
        mk = masks[:, lo:hi].bool()
        # non-varying columns map to an always-off sentinel column m
        mk = torch.cat([mk, zero_col.expand(b, hi - lo, 1)],
                       dim=2)[:, :, col_to_mask_col]
        rows = torch.where(
            mk[:, :, None, :], X64[:, None, None, :], bg64[None, None, :, :]
        )                                                 # (b, sc, N, D)
        ey[:, lo:hi] = torch.einsum("bsno,n->bso", forward(rows), wbg64)
    return ey


class _Backend:
    """What the three families share: the verification-mode constants, the
    logged-once fallback reason, the per-bucket group limit and the fp64
    blend around the family's forward."""

    _fallback_msg = ""
    max_groups = None        # varying groups one fused launch supports
    pack = None

    def __init__(self, gpu):
        self.gpu = gpu
        self.fused = False   # True when a fused kernel serves this engine
        self.kernel = None   # its name; None on the torch-module path
        self._logged = False

    def _load_f64_consts(self) -> bool:
        """Verification mode (predict_dtype 'fp64'): the unrounded fit-time
        constants. Returns whether the mode is on."""
        eng = self.gpu.engine
        if eng.kernels.predict_dtype != "fp64":
            return False
        for name, src in (("bg64", eng.background), ("wbg64", eng.bg_weights),
                          ("fnull64", eng.fnull)):
            setattr(self, name, torch.tensor(
                src, dtype=torch.float64, device=self.gpu.device))
        return True

    def _log_fallback(self, reason):
        if not self._logged:
            logger.info(self._fallback_msg, reason)
            self._logged = True

    def forward_f64(self, rows):
        with torch.no_grad():
            return self.mod64(rows)

    def _forward_blend(self, rows):
        p = self.forward_f64(rows.reshape(-1, rows.shape[-1]))
        return p.view(*rows.shape[:-1], -1)

    def ey_f64(self, masks, X_dev, varying):
        """Verification path: explicit masked blend + the fp64 forward on
        the SAME device masks."""
        g = self.gpu
        vmap = np.full(g.n_groups, masks.shape[2], dtype=np.int64)
        vmap[np.asarray(varying)] = np.arange(len(varying))
        colk = torch.tensor(vmap[g.engine._col_group], device=g.device)
        return blend_ey_f64(masks, X_dev.double(), self.bg64, self.wbg64,
                            colk, self._forward_blend, g.n_out, self.f64_width)

    def ey_fused(self, masks, X_dev, varying):
        """ey (B, S, n_out) from the fused kernel, or None when the bucket
        is outside its envelope (reason logged once per engine)."""
        if self.max_groups is not None and len(varying) > self.max_groups:
            self._log_fallback(
                f"{len(varying)} varying groups (supported: <= "
                f"{self.max_groups})"
            )
            return None
        return self._launch(masks, X_dev, varying)

    def workspace_bytes_per_instance(self, g: int) -> int:
        return 0

    def _cached_bg_image(self, varying, build):
        """Background operand image of a varying pattern (8 patterns kept)."""
        key = np.asarray(varying).tobytes()
        img = self.bg_img.get(key)
        if img is None:
            if len(self.bg_img) >= 8:
                self.bg_img.clear()
            img = self.bg_img[key] = build()
        return img


class MlpBackend(_Backend):
    """MLPPredictor: fused_predict_mlp (K4m) with the torch module as the
    out-of-envelope fallback."""

    _fallback_msg = ("MLPPredictor runs on the torch-module path, not the "
                     "fused MLP kernel: %s")
    max_groups = mlp_pack.MAX_GROUPS

    def __init__(self, gpu, predictor):
        super().__init__(gpu)
        kc = gpu.engine.kernels
        if kc.predict_dtype not in ("fp32", "bf16", "fp64"):
            raise ValueError(
                f"predict_dtype={kc.predict_dtype!r} is not available for "
                "MLPPredictor; supported: 'fp32', 'bf16' (fused MLP kernel) "
                "and 'fp64' (verification)"
            )
        W, b, self.hid, self.act = predictor.mlp_params()
        self.W64, self.b64 = (
            [torch.tensor(np.asarray(v), dtype=torch.float64,
                          device=gpu.device) for v in vs] for vs in (W, b))
        self.f64_width = max([gpu.D] + [w.shape[0] for w in self.W64])
        # every module-path consumer (fallback, sample-sharded, autocast)
        # keeps working; a private copy so the predictor's own stays on CPU
        self.module = copy.deepcopy(predictor.torch_module()).to(gpu.device)
        if self._load_f64_consts():
            return
        dtype = torch.bfloat16 if kc.predict_dtype == "bf16" else torch.float32
        reason = (None if kc.fused_predict
                  else "kernels.fused_predict is off")
        reason = reason or mlp_pack.envelope_reason(W, self.hid, dtype)
        if reason is not None:
            self._log_fallback(reason)
            return
        self.pack = mlp_pack.pack_mlp_weights(W, b, dtype, gpu.device)
        bg64 = gpu.bg.double()
        # fit-time constants shared by all instances
        self.bgpart1 = mlp_pack.group_parts(
            self.pack, bg64, gpu.col_group, gpu.n_groups)   # (N, H1pad, G)
        self.base1 = mlp_pack.base1(self.pack, bg64)        # (N, H1pad)
        self.bg_img = {}
        self.fused, self.kernel = True, "mlp"

    def forward_f64(self, rows):
        """fp64 torch forward from the fp64 weights."""
        h = rows.double()
        for w, b in zip(self.W64[:-1], self.b64[:-1]):
            h = h @ w.T + b
            if self.hid == "relu":
                h = torch.relu(h)
            elif self.hid == "tanh":
                h = torch.tanh(h)
        z = h @ self.W64[-1].T + self.b64[-1]
        if self.act == "softmax":
            return torch.softmax(z, dim=-1)
        if self.act == "sigmoid":
            return torch.sigmoid(z)
        return z

    _forward_blend = forward_f64      # takes the (b, sc, N, D) rows as they are

    def _launch(self, masks, X_dev, varying):
        """K4m. Only ey (B,S,n_out) reaches HBM; the workspaces are the
        first-layer operand images xp1 (B,H1pad,Mpad) and bgp1n
        (N,H1pad,Mpad), the latter cached per varying pattern."""
        g, pack = self.gpu, self.pack
        b, s, m = masks.shape
        vidx = torch.tensor(varying, dtype=torch.int64, device=g.device)
        bgp1n = self._cached_bg_image(varying, lambda: mlp_pack.first_layer_image(
            pack, self.bgpart1, vidx, negate=True))
        xparts = mlp_pack.group_parts(
            pack, X_dev.double(), g.col_group, g.n_groups)
        xp1 = mlp_pack.first_layer_image(pack, xparts, vidx)
        ey = g._buf("ey", (b, s, g.n_out))
        g.ext.fused_predict_mlp(
            masks.contiguous(), xp1, bgp1n, self.base1, pack["hidden_w"],
            pack["hidden_b"], pack["wout"], pack["bout"], g.bg_w, ey,
            mlp_pack.ACT_CODE[self.act], 0,
        )
        return ey

    def workspace_bytes_per_instance(self, g):
        if not self.fused:
            return 0
        # fp64 group parts (D x G indicator product and H1pad x G result)
        # + the xp1 operand image (H1pad x Mpad)
        h1 = self.pack["hpad"][0]
        return 8 * g * (self.gpu.D + 2 * h1) + 4 * h1 * (g + 31)


class TreeBackend(_Backend):
    """TreeEnsemblePredictor: fused_predict_trees (K4t, ``kernel == 'bits'``)
    or fused_predict_trees_walk (K4w, ``'walk'``) with the gather traversal
    torch module as the out-of-envelope fallback. A routed ensemble
    (tree_params() carries "routing": missing values and categorical splits)
    takes the same three paths: the modules and decision_bits encode raw rows
    themselves, the walk kernel reads rows encoded once (the background at
    fit, the instances per call)."""

    _fallback_msg = ("TreeEnsemblePredictor runs on the torch-module path, "
                     "not the fused tree kernel: %s")

    def __init__(self, gpu, predictor):
        super().__init__(gpu)
        kc = gpu.engine.kernels
        if kc.predict_dtype not in ("fp32", "fp64"):
            raise ValueError(
                f"predict_dtype={kc.predict_dtype!r} is not available for "
                "TreeEnsemblePredictor (a tree has nothing to round); "
                "supported: 'fp32' (fused tree kernel) and 'fp64' "
                "(verification)"
            )
        if kc.module_autocast == "bf16":
            raise ValueError(
                "module_autocast='bf16' is not available for "
                "TreeEnsemblePredictor: features rounded to bf16 would flip "
                "split decisions on the torch-module path"
            )
        params = predictor.tree_params()
        # fp64 tables on the device: per-instance totals and verification
        self.mod64 = predictor.build_module(torch.float64).to(gpu.device)
        self.f64_width = max(gpu.D, 4 * self.mod64.roots.shape[0])
        # every module-path consumer (fallback, sample-sharded) keeps
        # working; a fresh module, so the caller's predictor is not touched
        self.module = predictor.build_module().to(gpu.device)
        if self._load_f64_consts():
            return
        col_group = gpu.engine._col_group
        reason = (None if kc.fused_predict
                  else "kernels.fused_predict is off")
        walk = False
        if reason is None:
            reason = tree_pack.envelope_reason(params)
            if reason is not None:
                # beyond one u64 of split decisions per tree: the walk kernel
                walk_reason = tree_pack.walk_envelope_reason(
                    params, gpu.D, gpu.n_groups)
                walk = walk_reason is None
                reason = None if walk else f"{reason}; {walk_reason}"
        if reason is not None:
            self._log_fallback(reason)
        elif walk:
            self.pack = tree_pack.pack_trees_walk(params, col_group, gpu.device)
            # routed tables: the background as the nodes see it
            self.bg_enc = tree_pack.encode_rows(self.pack, gpu.bg)
            self.fused, self.kernel = True, "walk"
        else:
            self.pack = tree_pack.pack_trees(params, col_group, gpu.device)
            # fit-time constant shared by all instances: the background
            # rows' split decisions, one u64 per (row, tree)
            self.dbg = tree_pack.decision_bits(self.pack, gpu.bg)
            self.fused, self.kernel = True, "bits"

    def _launch(self, masks, X_dev, varying):
        """K4t / K4w. Only ey (B,S,n_out) reaches HBM; the per-call operands
        are the group -> varying-index table and, for the bit-register
        kernel, the instances' packed decisions dx (B,T)."""
        g, pack = self.gpu, self.pack
        b, s, m = masks.shape
        vmap_h = np.full(g.n_groups, -1, dtype=np.int32)
        vmap_h[np.asarray(varying)] = np.arange(m, dtype=np.int32)
        vmap = torch.tensor(vmap_h, device=g.device)
        ey = g._buf("ey", (b, s, g.n_out))
        if self.kernel == "walk":
            # K4w reads the float32 rows themselves (encoded, for routed
            # tables): no decision bits
            return tree_pack.fused_predict_walk(
                g.ext, pack, masks.contiguous(), vmap,
                tree_pack.encode_rows(pack, X_dev), self.bg_enc, g.bg_w, ey,
            )
        dx = tree_pack.decision_bits(pack, X_dev)
        return tree_pack.fused_predict(
            g.ext, pack, masks.contiguous(), vmap, dx, self.dbg, g.bg_w, ey,
        )

    def workspace_bytes_per_instance(self, g):
        if self.kernel != "bits":
            return 0     # the walk kernel reads x itself
        # packed decisions dx plus the (T, 64) comparison image behind them
        return self.pack["n_trees"] * (8 + 64 * 9)


class KernelMachineBackend(_Backend):
    """KernelMachinePredictor: fused_predict_kernelmachine (K4k) with the
    GEMM-form torch module as the out-of-envelope fallback.
    MulticlassSVCPredictor comes through the same hook: its "ovr" and
    "coupling" activations launch fused_predict_kernelmachine_pairs (K4kp)
    from km_pack.fused_predict, and ey has n_out = K columns. The fused
    workspaces are bounded per launch (km_pack.WORKSPACE_BYTES), not per
    instance."""

    _fallback_msg = ("KernelMachinePredictor runs on the torch-module path, "
                     "not the fused kernel-machine kernel: %s")
    max_groups = km_pack.MAX_GROUPS

    def __init__(self, gpu, predictor):
        super().__init__(gpu)
        kc = gpu.engine.kernels
        if kc.predict_dtype not in ("fp32", "fp64"):
            raise ValueError(
                f"predict_dtype={kc.predict_dtype!r} is not available for "
                "KernelMachinePredictor (a bf16 distance under an "
                "exponential is not a usable mode); supported: 'fp32' "
                "(fused kernel-machine kernel) and 'fp64' (verification)"
            )
        if kc.module_autocast == "bf16":
            raise ValueError(
                "module_autocast='bf16' is not available for "
                "KernelMachinePredictor: the distance expansion on the "
                "torch-module path cancels, and bf16 leaves nothing of it"
            )
        params = predictor.kernel_machine_params()
        # fp64 module on the device: per-instance totals and verification
        self.mod64 = predictor.build_module(torch.float64).to(gpu.device)
        self.f64_width = max(gpu.D, int(np.asarray(params["alpha"]).shape[1]))
        # every module-path consumer (fallback, sample-sharded) keeps
        # working; a fresh module, so the caller's predictor is not touched
        self.module = predictor.build_module().to(gpu.device)
        if self._load_f64_consts():
            return
        reason = (None if kc.fused_predict
                  else "kernels.fused_predict is off")
        reason = reason or km_pack.envelope_reason(params)
        if reason is not None:
            self._log_fallback(reason)
            return
        self.pack = km_pack.pack_machine(
            params, gpu.engine._col_group, gpu.n_groups, gpu.device)
        # fit-time constants shared by all instances
        self.bgparts = km_pack.group_parts(self.pack, gpu.bg.double())  # (N,V,G)
        self.base = km_pack.base(self.pack, self.bgparts)               # (N,Vpad)
        self.bg_img = {}
        self.fused, self.kernel = True, "kernelmachine"

    def _launch(self, masks, X_dev, varying):
        """K4k. Only ey (B,S,n_out) reaches HBM; the workspaces are the
        operand images xp (B,Vpad,Mpad) and bgpn (N,Vpad,Mpad), the latter
        cached per varying pattern. The bucket is split along B so that one
        launch's workspaces stay within ``km_pack.WORKSPACE_BYTES``."""
        g, pack = self.gpu, self.pack
        b, s, m = masks.shape
        vidx = torch.tensor(varying, dtype=torch.int64, device=g.device)
        bgpn = self._cached_bg_image(varying, lambda: km_pack.image(
            pack, self.bgparts, vidx, negate=True))
        masks = masks.contiguous()
        ey = g._buf("ey", (b, s, g.n_out))
        step = km_pack.instances_per_launch(pack, g.D, m)
        X64 = X_dev.double()
        for lo in range(0, b, step):
            hi = min(lo + step, b)
            xp = km_pack.image(
                pack, km_pack.group_parts(pack, X64[lo:hi]), vidx)
            km_pack.fused_predict(
                g.ext, pack, masks[lo:hi], xp, bgpn, self.base, g.bg_w,
                ey[lo:hi])
        return ey
