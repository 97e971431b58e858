"""Operand images for the fused kernel-machine predict kernel
(``fused_predict_kernelmachine``).

Everything here is plain torch on small tensors: the padded parameter copies
are built once per engine, the images once per bucket. All images are
computed in fp64 and rounded once to fp32.

The fold, with k over the varying groups of a bucket:

  pre[s,n,v] = base[n,v] + sum_k mask[s,k] (xp[b,v,k] - bgp[n,v,k])

  rbf :  part[r,v,g] = sum_{j in g} (row[r,j] - sv[v,j])^2   base = |bg[n]-sv[v]|^2
  poly:  part[r,v,g] = sum_{j in g}  row[r,j] sv[v,j]        base = bg[n].sv[v]

Layouts (k-contiguous, matching ``ops/hip/km_kernels.hip``):

  xp     (B, Vpad, Mpad) f32   ``group_parts`` of the instances, varying groups
  bgpn   (N, Vpad, Mpad) f32   the same of the background rows, NEGATED
  base   (N, Vpad) f32         sum of a background row's parts over ALL groups
  alpha  (16, Vpad) f32        dual coefficients; intercept (16) f32
  prob_a, prob_b (16) f32      Platt parameters per pair (one-vs-one epilogue)

Support vectors are zero-padded to a multiple of 16 and the varying-group
count to a multiple of 16. A padding support vector has all-zero images and
base, so its ``pre`` is exactly 0 and its kernel value finite (1 for rbf,
``coef0 ** degree`` for poly), and it carries ``alpha = 0``.
"""
from __future__ import annotations

import numpy as np

MAX_SV = 2048
MAX_NOUT = 8
MAX_GROUPS = 64
MAX_DEGREE = 8
# one-vs-one epilogue (MulticlassSVCPredictor, "ovr" / "coupling"): the pair
# decisions are the rows of the 16-row accumulator tile, of which row 15 idles
MAX_PAIRS = 15
MAX_CLASSES = 6

# Upper bound for the per-call workspaces of one kernel launch: the xp image
# and the fp64 intermediates behind it. The engine splits a bucket along B
# so that a launch stays below it.
WORKSPACE_BYTES = 256 << 20

ACT_CODE = {"none": 0, "sigmoid": 1, "softmax": 2, "ovr": 3, "coupling": 4}
PAIR_ACTS = ("ovr", "coupling")
KERNEL_CODE = {"rbf": 0, "poly": 1}


def _pad_to(n: int, k: int) -> int:
    return (n + k - 1) // k * k


def envelope_reason(params: dict):
    """None when the machine fits the fused kernel, else a one-line reason.
    (The varying-group count is a property of the bucket, not of the
    machine: the engine checks it per call.)"""
    if params["kernel"] not in KERNEL_CODE:
        return f"kernel {params['kernel']!r} (supported: rbf, poly)"
    n_out, n_sv = np.asarray(params["alpha"]).shape
    if _pad_to(n_sv, 16) > MAX_SV:
        return f"{n_sv} support vectors (supported: <= {MAX_SV})"
    if params["activation"] in PAIR_ACTS:
        k = int(params["n_classes"])
        if k > MAX_CLASSES or n_out > MAX_PAIRS:
            return f"{k} classes (supported: <= {MAX_CLASSES})"
    elif n_out > MAX_NOUT:
        return f"n_out {n_out} (supported: <= {MAX_NOUT})"
    if params["kernel"] == "poly" and params["degree"] > MAX_DEGREE:
        return f"degree {params['degree']} (supported: <= {MAX_DEGREE})"
    return None


def pack_machine(params: dict, col_group, n_groups: int, device) -> dict:
    """Padded device copies of the parameters. No envelope check: the kernel
    binding is the one place that refuses unsupported shapes."""
    import torch as t

    sv = t.as_tensor(np.asarray(params["support_vectors"], dtype=np.float64),
                     device=device)
    alpha = np.asarray(params["alpha"], dtype=np.float64)
    icpt = np.asarray(params["intercept"], dtype=np.float64).reshape(-1)
    n_out, n_sv = alpha.shape
    vpad = _pad_to(n_sv, 16)
    al = t.zeros(16, vpad, dtype=t.float64, device=device)
    al[: min(n_out, 16), :n_sv] = t.as_tensor(alpha[:16], device=device)
    ic = t.zeros(16, dtype=t.float64, device=device)
    ic[: min(n_out, 16)] = t.as_tensor(icpt[:16], device=device)
    d = sv.shape[1]
    cg = t.as_tensor(np.asarray(col_group), dtype=t.int64, device=device)
    onehot = t.zeros(d, n_groups, dtype=t.float64, device=device)
    onehot[t.arange(d, device=device), cg] = 1.0
    pairs = {}
    if params["activation"] in PAIR_ACTS:
        # the epilogue's operands: K and, for coupling, the Platt parameters
        # (zero-padded; the kernel reads entries below P only)
        prob = t.zeros(2, 16, dtype=t.float64, device=device)
        if params["activation"] == "coupling":
            for r, name in enumerate(("prob_a", "prob_b")):
                v = np.asarray(params[name], dtype=np.float64).reshape(-1)
                prob[r, : min(v.shape[0], 16)] = t.as_tensor(v[:16], device=device)
        pairs = {"n_classes": int(params["n_classes"]),
                 "prob_a": prob[0].float().contiguous(),
                 "prob_b": prob[1].float().contiguous()}
    return {
        **pairs,
        "kernel": params["kernel"], "gamma": float(params["gamma"]),
        "coef0": float(params["coef0"]), "degree": int(params["degree"]),
        "act": params["activation"], "n_out": n_out, "n_sv": n_sv,
        "vpad": vpad, "sv": sv, "onehot": onehot, "n_groups": n_groups,
        "alpha": al.float().contiguous(), "intercept": ic.float().contiguous(),
    }


def group_parts(pack: dict, rows64):
    """part[r, v, g] (fp64, ``(R, V, G)``): the share of group g in the
    squared distance (rbf) or the dot product (poly) between row r and
    support vector v."""
    sv = pack["sv"]
    if pack["kernel"] == "rbf":
        e = rows64[:, None, :] - sv[None, :, :]
        e = e * e
    else:
        e = rows64[:, None, :] * sv[None, :, :]
    return e @ pack["onehot"]                       # (R, V, D) @ (D, G)


def image(pack: dict, parts64, vidx, negate: bool = False):
    """Select the varying groups ``vidx`` of a ``group_parts`` result and
    zero-pad both axes -> (R, Vpad, Mpad) f32."""
    import torch as t

    m = int(vidx.shape[0])
    mpad = _pad_to(m, 16)
    img = t.zeros(parts64.shape[0], pack["vpad"], mpad, dtype=t.float32,
                  device=parts64.device)
    sel = parts64[:, :, vidx]
    img[:, : pack["n_sv"], :m] = (-sel if negate else sel).float()
    return img


def base(pack: dict, parts64):
    """Whole-row term of each background row: its parts summed over ALL
    groups (the non-varying ones stay with the background) -> (N, Vpad) f32."""
    import torch as t

    out = t.zeros(parts64.shape[0], pack["vpad"], dtype=t.float32,
                  device=parts64.device)
    out[:, : pack["n_sv"]] = parts64.sum(dim=2).float()
    return out


def instances_per_launch(pack: dict, d: int, m: int) -> int:
    """Instances whose xp image and fp64 intermediates stay within
    ``WORKSPACE_BYTES``."""
    v = pack["n_sv"]
    per_inst = 8 * v * (2 * d + pack["n_groups"] + m) \
        + 4 * pack["vpad"] * _pad_to(m, 16)
    return max(1, WORKSPACE_BYTES // per_inst)


def fused_predict(ext, pack: dict, masks, xp, bgpn, base_img, wbg, ey):
    """One launch of ``fused_predict_kernelmachine`` (or, for the one-vs-one
    activations, ``fused_predict_kernelmachine_pairs``); returns ``ey``."""
    if pack["act"] in PAIR_ACTS:
        ext.fused_predict_kernelmachine_pairs(
            masks, xp, bgpn, base_img, pack["alpha"], pack["intercept"],
            pack["prob_a"], pack["prob_b"], wbg, ey,
            KERNEL_CODE[pack["kernel"]], pack["gamma"], pack["coef0"],
            pack["degree"], ACT_CODE[pack["act"]], pack["n_classes"],
            pack["n_out"],
        )
        return ey
    ext.fused_predict_kernelmachine(
        masks, xp, bgpn, base_img, pack["alpha"], pack["intercept"], wbg, ey,
        KERNEL_CODE[pack["kernel"]], pack["gamma"], pack["coef0"],
        pack["degree"], ACT_CODE[pack["act"]],
    )
    return ey
