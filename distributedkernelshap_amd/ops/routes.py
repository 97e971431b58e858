"""Which kernel a bucket gets: pure functions of plain Python values.

No torch and no engine state, so every boundary is testable on a CPU
(``tests/test_routes.py``). ``kc`` is a ``KernelConfig`` (or anything with
its ``predict_dtype`` / ``fused_predict`` / ``wls_mode`` attributes), ``m``
the number of varying groups of the bucket, ``N`` the background rows.
"""
from __future__ import annotations

_BF16 = ("bf16", "bf16x2")


def pad_m(m: int) -> int:
    """Varying groups padded to the f32 MFMA's 4-deep k step."""
    return max(4, (m + 3) // 4 * 4)


def pad_n(n: int) -> int:
    """Background rows padded to the 16-column MFMA tile."""
    return (n + 15) // 16 * 16


def _fits_one_tile(n_out: int) -> bool:
    """Output counts the fused linear kernels are instantiated for."""
    return n_out in (1, 2, 4)


def graph_ok(kc, linear: bool, m: int, N: int, n_out: int,
             l1_active: bool) -> bool:
    """Whether a single-bucket call may be captured as a hipGraph: the
    envelope of the untiled u8-mask kernels with the kernel WLS. Unlike
    ``packed_ok`` it admits the bf16 predict dtypes and any ``(m-1)+n_out``
    (the captured body falls back to K3 + K7 there)."""
    return (
        linear
        and kc.fused_predict
        and kc.wls_mode in ("auto", "mfma")
        and 2 <= m <= 64
        and pad_n(N) <= 128
        and _fits_one_tile(n_out)
        and not l1_active
    )


def packed_ok(kc, linear: bool, m: int, N: int, n_out: int,
              l1_active: bool) -> bool:
    """Whether a bucket runs the packed pipeline (K2p, K0p, K3p, K7p):
    ``graph_ok`` narrowed to fp32 and to the one-wave MFMA solve,
    ``(m-1)+n_out <= 16``. Everything else keeps the u8-mask path."""
    return (
        graph_ok(kc, linear, m, N, n_out, l1_active)
        and kc.predict_dtype == "fp32"
        and (m - 1) + n_out <= 16
    )


def linear_predict_route(kc, m: int, N: int, n_out: int, act3: bool):
    """``(route, pairwise)`` of the eager bucket loop for a linear predictor
    on u8 masks. ``route`` is 'bf16', 'u8', 'tiled_bf16', 'tiled' or 'torch';
    ``pairwise`` says that ey carries the softmax pair (p0, p1) and the link
    takes log(p1) - log(p0)."""
    ok = kc.fused_predict and _fits_one_tile(n_out)
    bf = kc.predict_dtype in _BF16
    one_tile = pad_n(N) <= 128
    if ok and bf and m <= 32 and one_tile:
        return "bf16", False
    if ok and kc.predict_dtype == "fp32" and pad_m(m) <= 64 and one_tile:
        return "u8", False
    split = 2 if kc.predict_dtype == "bf16x2" else 1
    # the tiled bf16 kernel holds split x images x (128 x 40) bf16 in LDS
    if ok and bf and split * (1 if act3 else n_out) * 128 * 40 * 2 <= 65536:
        return "tiled_bf16", act3
    if ok:
        return "tiled", act3
    return "torch", act3


# Varying-group counts at which a captured graph and the eager loop run
# different kernels under a bf16 predict dtype: ``graph_predict_route`` gives
# 'u8' (fp32), ``linear_predict_route`` a tiled kernel. Kept as found; see
# TODO.md.
GRAPH_EAGER_BF16_GAP = range(33, 65)


def graph_predict_route(kc, m: int, n_out: int) -> str:
    """Route of the captured graph body, inside ``graph_ok`` and outside
    ``packed_ok``: the bf16 kernel up to 32 groups, else the u8 fp32 kernel
    whatever the dtype (narrower than ``linear_predict_route`` over
    ``GRAPH_EAGER_BF16_GAP``)."""
    if kc.predict_dtype in _BF16 and m <= 32 and _fits_one_tile(n_out):
        return "bf16"
    return "u8"


def sharded_predict_route(m: int, N: int, n_out: int) -> str:
    """Route of the sample-sharded path: the u8 kernel inside its envelope,
    the torch GEMM otherwise, whatever ``predict_dtype`` says."""
    if pad_m(m) <= 64 and pad_n(N) <= 128 and _fits_one_tile(n_out):
        return "u8"
    return "torch"


def pad_out(n_out: int) -> int:
    """Class count padded to the widths the wide linear kernel is
    instantiated for (4, 8, 12, 16)."""
    return (n_out + 3) // 4 * 4


def wide_linear_ok(kc, m: int, N: int, n_out: int) -> bool:
    """Whether a bucket of a linear predictor with 3, or 5 to 16, outputs
    runs the column-tile-streamed kernel (K4l). The eager bucket loop asks
    this first; ``linear_predict_route`` answers 'torch' for these output
    counts, an fp32 route whatever ``predict_dtype`` says, so the fp32 wide
    kernel serves the bf16 settings too. ``n_out == 4`` keeps its one-tile
    kernels."""
    return bool(
        kc.fused_predict
        and kc.predict_dtype in ("fp32",) + _BF16
        and 3 <= n_out <= 16
        and n_out != 4
        and 2 <= m
        and pad_m(m) <= 64
        and pad_n(N) <= 512
    )


def wls_output_chunks(linear: bool, n_out: int):
    """Column ranges ``[(lo, hi), ...]`` of the outputs solved together. The
    WLS problems of different outputs share masks and weights and differ only
    in the right-hand side, so 9 to 16 outputs of a linear predictor go
    through the solvers (at most 8 outputs a call) as two chunks; everything
    else is one chunk, as before."""
    if linear and 9 <= n_out <= 16:
        return [(0, 8), (8, n_out)]
    return [(0, n_out)]


def wls_route(kc, m: int, n_out: int) -> str:
    """'kernel' (K7), 'gram' (MFMA Gram build + fp64 solve) or 'torch'.
    fp32 Gram conditioning degrades with m (Shapley kernel weights span
    orders of magnitude): the MFMA solve covers (m-1)+n_out <= 16, the
    scalar fp32 kernel up to m = 24, larger m goes to an fp64 solve."""
    if (kc.wls_mode != "torch" and m >= 2 and n_out <= 8
            and (m - 1 + n_out <= 16 or m <= 24)):
        return "kernel"
    if kc.wls_mode in ("auto", "mfma") and m <= 513 and n_out <= 8:
        return "gram"
    return "torch"
