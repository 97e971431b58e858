"""Operand images for the fused MLP predict kernel (``fused_predict_mlp``).

Everything here is plain torch on small tensors: the padded weight copies
are built once per engine, the first-layer images once per bucket. All
images are computed in fp64 and rounded once to the kernel's operand dtype.

Layouts (k-contiguous, matching ``ops/hip/mlp_kernels.hip``):

  xp1    (B, H1pad, Mpad)   xp1[b,h,k]  =  sum_{j in group k} x[b,j] W1[h,j]
  bgp1n  (N, H1pad, Mpad)   the same sum over bg[n], NEGATED
  base1  (N, H1pad) f32     W1 bg[n] + b1
  hidden_w[l] (Hpad[l+1], Hpad[l]),  hidden_b[l] (Hpad[l+1]) f32
  wout   (nsplit, 16, Hpad[-1])   output layer padded to 16 rows; the bf16
                            variant carries a hi+lo pair (f32-grade)
  bout   (16) f32

Hidden widths and the varying-group count are zero-padded to the MFMA k
depth of one operand load: 16 (fp32) or 32 (bf16).
"""
from __future__ import annotations

from typing import Sequence

import numpy as np

MAX_HIDDEN_LAYERS = 3
MAX_WIDTH = 256
MAX_NOUT = 8
MAX_GROUPS = 64

ACT_CODE = {"none": 0, "sigmoid": 1, "softmax": 2}


def k_depth(dtype) -> int:
    import torch

    return 32 if dtype == torch.bfloat16 else 16


def _pad_to(n: int, k: int) -> int:
    return (n + k - 1) // k * k


def envelope_reason(weights: Sequence[np.ndarray], hidden_activation: str,
                    dtype=None):
    """None when the network fits the fused kernel, else a one-line reason."""
    nhid = len(weights) - 1
    if nhid < 1 or nhid > MAX_HIDDEN_LAYERS:
        return f"{nhid} hidden layers (supported: 1-{MAX_HIDDEN_LAYERS})"
    if hidden_activation != "relu":
        return f"hidden activation {hidden_activation!r} (supported: relu)"
    kd = 16 if dtype is None else k_depth(dtype)
    widest = max(_pad_to(w.shape[0], kd) for w in weights[:-1])
    if widest > MAX_WIDTH:
        return f"hidden width {widest} after padding (supported: <= {MAX_WIDTH})"
    if weights[-1].shape[0] > MAX_NOUT:
        return f"n_out {weights[-1].shape[0]} (supported: <= {MAX_NOUT})"
    return None


def pack_mlp_weights(weights, biases, dtype, device) -> dict:
    """Padded device copies of the weights in operand dtype ``dtype``
    (torch.float32 or torch.bfloat16). No envelope check: the kernel
    binding is the one place that refuses unsupported shapes."""
    import torch as t

    kd = k_depth(dtype)
    ws = [t.as_tensor(np.asarray(w, dtype=np.float64), device=device) for w in weights]
    bs = [t.as_tensor(np.asarray(b, dtype=np.float64), device=device) for b in biases]
    hpad = [_pad_to(w.shape[0], kd) for w in ws[:-1]]
    d = ws[0].shape[1]
    w1 = t.zeros(hpad[0], d, dtype=t.float64, device=device)
    w1[: ws[0].shape[0]] = ws[0]
    b1 = t.zeros(hpad[0], dtype=t.float64, device=device)
    b1[: bs[0].shape[0]] = bs[0]
    hidden_w, hidden_b = [], []
    for l in range(1, len(ws) - 1):
        w = t.zeros(hpad[l], hpad[l - 1], dtype=t.float64, device=device)
        w[: ws[l].shape[0], : ws[l].shape[1]] = ws[l]
        b = t.zeros(hpad[l], dtype=t.float64, device=device)
        b[: bs[l].shape[0]] = bs[l]
        hidden_w.append(w.to(dtype).contiguous())
        hidden_b.append(b.float().contiguous())
    n_out = ws[-1].shape[0]
    wo = t.zeros(16, hpad[-1], dtype=t.float64, device=device)
    wo[: min(n_out, 16), : ws[-1].shape[1]] = ws[-1][:16]
    bo = t.zeros(16, dtype=t.float64, device=device)
    bo[: min(n_out, 16)] = bs[-1][:16]
    if dtype == t.bfloat16:
        hi = wo.to(t.bfloat16)
        lo = (wo - hi.double()).to(t.bfloat16)
        wout = t.stack([hi, lo]).contiguous()
    else:
        wout = wo.to(dtype)[None].contiguous()
    return {
        "dtype": dtype, "hpad": hpad, "n_out": n_out, "w1": w1, "b1": b1,
        "hidden_w": hidden_w, "hidden_b": hidden_b, "wout": wout,
        "bout": bo.float().contiguous(),
    }


def group_parts(pack: dict, rows64, col_group, n_groups: int):
    """part[r, h, g] = sum_{j in group g} rows[r, j] * W1[h, j]  (fp64)."""
    import torch as t

    d = rows64.shape[1]
    onehot = t.zeros(d, n_groups, dtype=t.float64, device=rows64.device)
    onehot[t.arange(d, device=rows64.device), col_group] = 1.0
    # (R, D, G) scaled indicator, then one batched matmul with W1 (H1, D)
    return t.matmul(pack["w1"][None], rows64[:, :, None] * onehot[None])


def first_layer_image(pack: dict, parts64, vidx, negate: bool = False):
    """Select the varying groups ``vidx`` of a ``group_parts`` result and
    zero-pad the k axis to the operand depth -> (R, H1pad, Mpad)."""
    import torch as t

    m = int(vidx.shape[0])
    mpad = _pad_to(m, k_depth(pack["dtype"]))
    img = t.zeros(parts64.shape[0], parts64.shape[1], mpad,
                  dtype=pack["dtype"], device=parts64.device)
    sel = parts64[:, :, vidx]
    img[:, :, :m] = (-sel if negate else sel).to(pack["dtype"])
    return img


def base1(pack: dict, bg64):
    """W1 bg[n] + b1 -> (N, H1pad) f32."""
    return (bg64 @ pack["w1"].T + pack["b1"][None]).float().contiguous()
