"""float64 reference of the fused linear predict and the tolerance derived
from its operands. A plain helper module: pytest does not collect it.

    ey[b,s,o] = sum_n w[n] * act( base[o,n] + sum_k mask[b,s,k] * diff[b,o,k,n] )

act 0 = identity, 1 = sigmoid, 2 = softmax over o, 3 = binary softmax from one
logit-difference image: p1 = sigmoid(z), p0 = sigmoid(-z) (never 1 - p1, so a
saturated p0 keeps its relative accuracy).
"""
import torch

EPS = 2.0 ** -24            # fp32 unit roundoff
ZSCALE = 6.0                # |base| + sum_k |diff_k| per column, probability acts


def fp64_reference(masks, diff, base, wbg, act):
    """masks (B,S,m) 0/1; diff (B,OIMG,K>=m,N); base (OIMG,N); wbg (N).
    Returns z (B,S,OIMG,N), p (B,S,n_out,N) and ey (B,S,n_out), all float64."""
    m = masks.shape[2]
    z = torch.einsum("bsk,bokn->bson", masks.double(), diff[:, :, :m].double())
    z = z + base.double()[None, None]
    if act == 0:
        p = z
    elif act == 1:
        p = torch.sigmoid(z)
    elif act == 2:
        p = torch.softmax(z, dim=2)
    elif act == 3:
        p = torch.stack([torch.sigmoid(-z[:, :, 0]), torch.sigmoid(z[:, :, 0])],
                        dim=2)
    else:
        raise ValueError(act)
    ey = torch.einsum("bson,n->bso", p, wbg.double())
    return z, p, ey


def lipschitz(n_out, act):
    """Bound on |d act / d z| summed the way a z error enters one output."""
    if act == 0:
        return 1.0
    if act == 2 and n_out > 2:
        return 0.5          # general softmax
    return 0.25             # sigmoid, act 3, binary softmax


def column_bound(diff, base):
    """max over columns of |base| + sum_k |diff_k|  (bounds every |z|)."""
    return (base.double().abs()[None]
            + diff.double().abs().sum(dim=2)).max().item()


def derived_tolerance(diff, base, wbg, p, n, n_out, act, k_terms):
    """tol = L*dz + (N+4) * 2^-24 * sum|w| * max|act| + 1e-6 with
    dz = (k_terms+1) * 2^-24 * max_col(|base| + sum_k |diff_k|): k_terms fp32
    additions of partial sums bounded by the column bound, one more for the
    base; N weighted adds plus the 4-step lane reduction; 1e-6 for the
    __expf / v_rcp epilogue."""
    dz = (k_terms + 1) * EPS * column_bound(diff, base)
    red = (n + 4) * EPS * wbg.double().abs().sum().item() * p.abs().max().item()
    return lipschitz(n_out, act) * dz + red + 1e-6
