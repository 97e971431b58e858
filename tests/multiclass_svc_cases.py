"""Kernel-level cases of the one-vs-one fused predict, shared by the CPU tests
(which measure the fp32 torch module on them: the yardstick for the GPU
bounds) and the GPU tests (which run the HIP kernel on them).

A case is an explicit blend fed to the numpy oracle, with non-uniform
background weights, as in ``test_gpu_kernel_machine.py``.
"""
import numpy as np

from distributedkernelshap_amd.models import MulticlassSVCPredictor

# the project's fused-predict bound
ATOL, RTOL = 2e-5, 1e-4
# ovr is discontinuous where a pair decision crosses 0: entries with a blended
# row whose |f_p| is below this are left out (about 30x the 3e-6 error in z)
OVR_MARGIN = 1e-4


def _chunked_groups(d, m):
    cuts = np.linspace(0, d, m + 1).round().astype(int)
    return [list(range(cuts[i], cuts[i + 1])) for i in range(m)]


# (D, groups, N, S, B, V, kernel, K, act, extra) — each the smallest shape
# that breaks one assumption
SHAPES = {
    # everything below one tile; a wave with no rows; ragged S
    1: (7, [[0], [1, 2], [3], [4, 5, 6]], 3, 70, 1, 5, "rbf", 3, "ovr", {}),
    # pair rows in all four lane quarters, row 15 idle; ragged V tile
    2: (9, _chunked_groups(9, 5), 19, 70, 1, 37, "rbf", 6, "coupling", {}),
    # 6 pairs straddle a lane-quarter boundary
    3: (9, _chunked_groups(9, 5), 19, 70, 1, 37, "poly", 4, "coupling",
        dict(degree=3, coef0=0.5)),
    # two sample tiles, N < waves, three k chunks
    4: (33, [[j] for j in range(33)], 2, 130, 1, 17, "rbf", 6, "ovr", {}),
    # batch stride
    5: (9, _chunked_groups(9, 5), 19, 70, 3, 37, "rbf", 3, "coupling", {}),
    # prob_a scaled so that most pair probabilities hit the 1e-7 clip
    6: (9, _chunked_groups(9, 5), 5, 70, 1, 37, "rbf", 4, "coupling",
        dict(prob_a_scale=400.0)),
    # the new class through the OLD entry point (P = 6 <= 8)
    7: (9, _chunked_groups(9, 5), 19, 70, 1, 37, "rbf", 4, "none", {}),
}


def problem(shape_id):
    d, groups, n, s, b, v, kernel, k, act, extra = SHAPES[shape_id]
    rng = np.random.Generator(np.random.Philox(key=[127, shape_id]))
    extra = dict(extra)
    scale = extra.pop("prob_a_scale", None)
    pred = MulticlassSVCPredictor.random(
        d, k, n_sv=v, kernel=kernel, seed=shape_id, activation=act, **extra)
    if scale is not None:
        pred = MulticlassSVCPredictor(
            pred.support_vectors, pred.alpha, pred.intercept, k, kernel=kernel,
            gamma=pred.gamma, activation=act, prob_a=scale * pred.prob_a,
            prob_b=pred.prob_b)
    x = rng.normal(size=(b, d))
    bg = rng.normal(size=(n, d))
    wbg = rng.uniform(0.2, 1.0, size=n)          # non-uniform
    wbg /= wbg.sum()
    col_group = np.empty(d, dtype=np.int64)
    for gi, g in enumerate(groups):
        col_group[g] = gi
    m = len(groups)
    masks = (rng.uniform(size=(b, s, m)) < 0.5).astype(np.uint8)
    return dict(pred=pred, x=x, bg=bg, wbg=wbg, masks=masks,
                col_group=col_group, n_groups=m)


def blend(p):
    """The explicit (B, S, N, D) blended rows."""
    on = p["masks"][:, :, p["col_group"]] != 0
    return np.where(on[:, :, None, :], p["x"][:, None, None, :],
                    p["bg"][None, None, :, :])


def reference(p, rows=None):
    """(B, S, n_out) fp64: the numpy oracle on the blended rows, reduced with
    the background weights."""
    rows = blend(p) if rows is None else rows
    b, s, n, d = rows.shape
    pr = p["pred"](rows.reshape(-1, d)).reshape(b, s, n, -1)
    return np.einsum("bsno,n->bso", pr, p["wbg"])


def module_fp32(p, rows=None):
    """The same through the fp32 torch module (rows rounded to fp32, the
    weighted reduction in fp64): the CPU stand-in for the kernel."""
    import torch

    rows = blend(p) if rows is None else rows
    b, s, n, d = rows.shape
    with torch.no_grad():
        pr = p["pred"].build_module()(
            torch.from_numpy(rows.reshape(-1, d)).float()).double().numpy()
    return np.einsum("bsno,n->bso", pr.reshape(b, s, n, -1), p["wbg"])


def ovr_keep(p, rows=None):
    """(B, S) bool: entries whose every blended row has all |f_p| >=
    OVR_MARGIN in fp64."""
    rows = blend(p) if rows is None else rows
    b, s, n, d = rows.shape
    f = p["pred"].raw(rows.reshape(-1, d)).reshape(b, s, n, -1)
    return (np.abs(f) >= OVR_MARGIN).all(axis=(2, 3))


_CASES = {}


def case(shape_id):
    """Problem, reference and (for ovr) the kept entries; computed once and
    shared, never mutated."""
    if shape_id not in _CASES:
        p = problem(shape_id)
        rows = blend(p)
        keep = ovr_keep(p, rows) if p["pred"].activation == "ovr" \
            else np.ones(rows.shape[:2], dtype=bool)
        _CASES[shape_id] = (p, reference(p, rows), keep)
    return _CASES[shape_id]
