"""The four u8-mask linear predict kernels (fused_predict_linear,
fused_predict_bf16, fused_predict_tiled, fused_predict_tiled_bf16) and the
bf16 operand builders, called directly and held to a float64 evaluation of
the same operands at the smallest shapes that reach each code path.

Tolerance (tests/linear_predict_reference.py), computed per case from the
operands and never from what the kernel returns:

    dz  = (K_terms + 1) * 2^-24 * max_col(|base| + sum_k |diff_k|)
    tol = L * dz + (N + 4) * 2^-24 * sum|w| * max|act| + 1e-6

K_terms = Mpad for the fp32 kernels and Mpad * split for the bf16 ones (a
0/1 x bf16 product is exact in fp32); L = 1 (identity), 1/4 (sigmoid, act 3,
binary softmax), 1/2 (general softmax); 1e-6 covers the __expf / v_rcp
epilogue. The bf16 kernels are compared with the float64 evaluation of the
DEQUANTISED operand (hi + lo) at that tolerance, and once more with the
unquantised fp32 operand at tol + L * u * max_col sum_k |diff_k|, u = 2^-8
for one image and 2^-16 for the hi + lo pair.

Every case prints its measured error beside the tolerance.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from linear_predict_reference import (  # noqa: E402
    ZSCALE, column_bound, derived_tolerance, fp64_reference, lipschitz,
)

DEV = "cuda"
NAN = float("nan")
KSTRIDE_BF = 40             # k stride of the untiled bf16 operand image


@pytest.fixture(scope="module")
def ext():
    from distributedkernelshap_amd.ops import load_extension

    return load_extension()


def _ceil(x, q):
    return (x + q - 1) // q * q


def _operands(b, s, m, n, n_out, act, seed, mpad, wsum=1.0, zscale=ZSCALE,
              bf16_headroom=False):
    """Random 0/1 masks, a randn diff image (B, OIMG, mpad, Npad) with zero
    pad slots, a randn base and non-uniform weights that sum to ``wsum``.
    For the probability activations |base| + sum_k |diff_k| <= zscale in
    every column (also after a bf16 rounding with ``bf16_headroom``)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    oimg = 1 if act == 3 else n_out
    npad = _ceil(n, 16)
    masks = (torch.rand(b, s, m, generator=g, device=DEV) > 0.5).to(torch.uint8)
    diff = torch.zeros(b, oimg, mpad, npad, device=DEV)
    diff[:, :, :m, :n] = torch.randn(b, oimg, m, n, generator=g, device=DEV)
    base = torch.zeros(oimg, npad, device=DEV)
    base[:, :n] = torch.randn(oimg, n, generator=g, device=DEV)
    if act != 0:
        f = zscale / column_bound(diff, base) * (1.0 - 2.0 ** -20)
        if bf16_headroom:
            f /= 1.0 + 2.0 ** -8
        diff *= f
        base *= f
    w = torch.rand(n, generator=g, device=DEV, dtype=torch.float64) + 0.1
    wbg = torch.zeros(npad, device=DEV)
    wbg[:n] = (w / w.sum() * wsum).float()
    return masks, diff, base, wbg


def _bf16_images(diff, split, kstride):
    """hi (+ lo) bf16 images of an fp32 (B, OIMG, Mpad, Npad) diff in the
    kernels' (B, split, OIMG, Npad, kstride) k-contiguous layout, and the
    float64 value of what they hold, back in (B, OIMG, Mpad, Npad)."""
    b, oimg, mpad, npad = diff.shape
    hi = diff.to(torch.bfloat16)
    imgs = [hi]
    deq = hi.double()
    if split == 2:
        lo = (diff - hi.float()).to(torch.bfloat16)
        imgs.append(lo)
        deq = deq + lo.double()
    out = torch.zeros(b, split, oimg, npad, kstride, dtype=torch.bfloat16,
                      device=DEV)
    for sp, img in enumerate(imgs):
        out[:, sp, :, :, :mpad] = img.permute(0, 1, 3, 2)
    return out, deq


def _run_linear(ext, masks, diff, base, wbg, n_out, act):
    b, s, _ = masks.shape
    ey = torch.full((b, s, n_out), NAN, device=DEV)
    ext.fused_predict_linear(masks, diff, base, wbg, ey, act)
    return ey


def _run_bf16(ext, masks, diffb, base, wbg, n_out, act):
    b, s, _ = masks.shape
    ey = torch.full((b, s, n_out), NAN, device=DEV)
    ext.fused_predict_bf16(masks, diffb, base, wbg, ey, act)
    return ey


def _run_tiled(ext, masks, diff, base, wbg, n_out, act, bf16=False):
    b, s, _ = masks.shape
    n_ntiles = (wbg.shape[0] + 127) // 128
    partial = torch.full((b, n_ntiles, s, n_out), NAN, device=DEV)
    ey = torch.full((b, s, n_out), NAN, device=DEV)
    fn = ext.fused_predict_tiled_bf16 if bf16 else ext.fused_predict_tiled
    fn(masks, diff, base, wbg, partial, ey, act)
    return ey


def _check(name, ey, masks, diff_ref, base, wbg, n, n_out, act, k_terms,
           extra=0.0):
    """ey against the float64 evaluation of diff_ref at the derived tolerance
    (+ extra). Returns measured / tolerance."""
    z, p, ref = fp64_reference(masks, diff_ref, base, wbg, act)
    if act != 0:
        assert z.abs().max().item() <= ZSCALE + 1e-9
    assert not bool(torch.isnan(ey).any()), f"{name}: NaN left in ey"
    tol = derived_tolerance(diff_ref, base, wbg, p, n, n_out, act, k_terms)
    tol += extra
    err = (ey.double() - ref).abs().max().item()
    print(f"{name}: max|ey-fp64|={err:.3e} tol={tol:.3e} ratio={err / tol:.3f}")
    assert err <= tol, (name, err, tol)
    return err / tol


def _check_bf16(name, ey, masks, diff, deq, base, wbg, n, n_out, act, mpad,
                split):
    """The dequantised operand at the derived tolerance, then the fp32
    operand with the quantisation term added."""
    _check(f"{name} vs dequantised", ey, masks, deq, base, wbg, n, n_out,
           act, mpad * split)
    u = 2.0 ** -8 if split == 1 else 2.0 ** -16
    quant = (lipschitz(n_out, act) * u
             * diff.double().abs().sum(dim=2).max().item())
    _check(f"{name} vs fp32 operand", ey, masks, diff, base, wbg, n, n_out,
           act, mpad * split, extra=quant)


# --------------------------------------------------------------------------- #
# fused_predict_linear: fp32 MFMA, whole diff image in LDS

# (b, s, m, n, n_out, act)
LINEAR_CASES = [
    (2, 1, 12, 37, 2, 1),       # one row: 63 of 64 sub-tile rows invalid
    (2, 15, 12, 37, 2, 1),      # less than one wave's 16 rows
    (2, 64, 12, 37, 2, 1),      # exactly one sub-tile
    (2, 65, 12, 37, 2, 1),      # a second sub-tile of one row
    (2, 513, 12, 37, 2, 1),     # a second 512-row tile of one row
    (2, 70, 1, 37, 2, 3),       # Mpad 4
    (2, 70, 64, 128, 2, 3),     # Mpad 64, one image, NT 8
    (2, 70, 12, 37, 4, 0),      # four images
    (2, 70, 12, 37, 4, 1),
    (2, 70, 12, 37, 4, 2),      # the general softmax branch
    (2, 70, 12, 128, 2, 1),     # NT 8, NSTRIDE 144
    (2, 70, 12, 16, 1, 0),      # NT 1: the second column half is empty
    (2, 70, 13, 37, 1, 1),      # Mpad 16 with three zero k slots
    (2, 70, 12, 37, 2, 2),      # binary softmax from two images
    (2, 70, 12, 37, 2, 0),
]


def _linear_case(ext, b, s, m, n, n_out, act, seed):
    mpad = max(4, _ceil(m, 4))
    masks, diff, base, wbg = _operands(b, s, m, n, n_out, act, seed, mpad)
    ey = _run_linear(ext, masks, diff, base, wbg, n_out, act)
    name = f"fused_predict_linear b={b} s={s} m={m} n={n} o={n_out} act={act}"
    return _check(name, ey, masks, diff, base, wbg, n, n_out, act, mpad)


@pytest.mark.parametrize("b,s,m,n,n_out,act", LINEAR_CASES)
def test_fused_predict_linear_vs_fp64(ext, b, s, m, n, n_out, act):
    _linear_case(ext, b, s, m, n, n_out, act, seed=1000 + s + m + n + act)


# (n_out, act, m, n, dynamic LDS bytes from the launcher's formula)
LINEAR_LDS_CASES = [
    (2, 1, 52, 128, 61440),     # just under 64 KiB
    (2, 1, 56, 128, 66048),
    (2, 1, 64, 128, 75264),
    (4, 2, 40, 100, 73920),     # 4-class softmax, 40 groups, 100 rows
    (4, 1, 64, 128, 150016),
]


@pytest.mark.parametrize("n_out,act,m,n,lds", LINEAR_LDS_CASES)
def test_fused_predict_linear_large_lds(ext, n_out, act, m, n, lds):
    """Shapes the engine dispatches whose dynamic LDS passes 48 and 64 KiB."""
    mpad, npad = _ceil(m, 4), _ceil(n, 16)
    nstride = npad + ((16 - (npad & 31)) & 31)
    assert (n_out * mpad * nstride + n_out * npad + npad) * 4 == lds
    _linear_case(ext, 2, 70, m, n, n_out, act, seed=2000 + m + n)


# --------------------------------------------------------------------------- #
# build_diff_bf16 / build_diff_bf16_tiled

def _bits(x):
    return x.view(torch.int16)


@pytest.mark.parametrize("o_img", [1, 2])
@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("layout", ["k40", "tiled32", "tiled96"])
def test_build_diff_bf16_bit_exact_and_pads_untouched(ext, layout, split, o_img):
    g = torch.Generator(device=DEV).manual_seed(40 + split + o_img)
    b, G, n, npad = 3, 9, 20, 32
    vidx = torch.tensor([0, 2, 3, 7, 8], dtype=torch.int64, device=DEV)
    m = vidx.shape[0]
    xp = torch.randn(b, G, o_img, generator=g, device=DEV)
    bgp = torch.randn(n, G, o_img, generator=g, device=DEV)
    kdim = {"k40": KSTRIDE_BF, "tiled32": 32, "tiled96": 96}[layout]
    sentinel = torch.tensor(7.0, dtype=torch.bfloat16, device=DEV)
    out = sentinel.expand(b, split, o_img, npad, kdim).contiguous()
    if layout == "k40":
        ext.build_diff_bf16(xp, bgp, vidx, out)
    else:
        ext.build_diff_bf16_tiled(xp, bgp, vidx, out)
    # v[b, o, n, k] = xp[b, vidx[k], o] - bgp[n, vidx[k], o]: one fp32
    # subtraction, so torch's result is the kernel's bit for bit
    v = (xp[:, vidx].permute(0, 2, 1)[:, :, None, :]
         - bgp[:, vidx].permute(2, 0, 1)[None])
    assert v.shape == (b, o_img, n, m) and v.dtype == torch.float32
    hi = v.to(torch.bfloat16)
    want = sentinel.expand(b, split, o_img, npad, kdim).contiguous()
    want[:, 0, :, :n, :m] = hi
    if split == 2:
        want[:, 1, :, :n, :m] = (v - hi.float()).to(torch.bfloat16)
        assert bool((want[:, 1, :, :n, :m] != 0).any())
    written = torch.zeros_like(want, dtype=torch.bool)
    written[:, :, :, :n, :m] = True
    assert bool((_bits(out)[~written] == _bits(sentinel)).all()), (
        "a pad slot (k >= m or n >= N) was written")
    nbad = int((_bits(out) != _bits(want)).sum().item())
    print(f"build_diff_bf16 {layout} split={split} O={o_img}: "
          f"{nbad} of {out.numel()} slots differ in bits")
    assert nbad == 0


# --------------------------------------------------------------------------- #
# fused_predict_bf16: one 32-deep bf16 MFMA over k, M <= 32

# (b, s, m, n, n_out, act, split)
BF16_CASES = [
    (2, 1, 1, 16, 1, 0, 1),
    (2, 65, 12, 37, 1, 1, 2),
    (2, 513, 31, 37, 2, 1, 1),
    (2, 65, 32, 128, 2, 2, 2),      # every k slot and every column tile used
    (2, 65, 12, 37, 2, 3, 1),
    (2, 65, 12, 37, 2, 3, 2),
    (2, 65, 12, 16, 4, 1, 1),
    (2, 65, 31, 37, 4, 2, 2),       # general softmax
    (2, 1, 32, 128, 2, 3, 2),
    (2, 513, 12, 37, 2, 2, 1),
    (2, 65, 12, 37, 1, 0, 2),
]


def _bf16_case(ext, b, s, m, n, n_out, act, split, seed):
    masks, diff, base, wbg = _operands(b, s, m, n, n_out, act, seed, 32,
                                       bf16_headroom=True)
    diffb, deq = _bf16_images(diff, split, KSTRIDE_BF)
    ey = _run_bf16(ext, masks, diffb, base, wbg, n_out, act)
    name = (f"fused_predict_bf16 b={b} s={s} m={m} n={n} o={n_out} act={act} "
            f"split={split}")
    _check_bf16(name, ey, masks, diff, deq, base, wbg, n, n_out, act, 32, split)


@pytest.mark.parametrize("b,s,m,n,n_out,act,split", BF16_CASES)
def test_fused_predict_bf16_vs_fp64(ext, b, s, m, n, n_out, act, split):
    _bf16_case(ext, b, s, m, n, n_out, act, split,
               seed=3000 + s + m + n + act + split)


@pytest.mark.parametrize("act,n,lds", [(2, 100, 73928), (1, 128, 84488)])
def test_fused_predict_bf16_large_lds(ext, act, n, lds):
    """Four images, hi + lo: the dynamic LDS passes 64 KiB."""
    npad = _ceil(n, 16)
    want = 2 * 4 * npad * KSTRIDE_BF * 2 + 2 + (4 * npad + npad) * 4
    assert _ceil(want, 4) + 4 == lds
    _bf16_case(ext, 2, 70, 30, n, 4, act, 2, seed=3500 + n)


# --------------------------------------------------------------------------- #
# fused_predict_tiled: fp32 MFMA, diff streamed in k chunks, 128-column tiles

# (b, s, m, n, n_out, act, wsum)
TILED_CASES = [
    (2, 1, 3, 16, 1, 0, 1.0),       # Mpad 16: one chunk, one row
    (2, 63, 3, 16, 1, 1, 1.0),
    (2, 63, 65, 130, 1, 2, 1.0),    # Mpad 80; a second column tile of 16
    (2, 577, 65, 130, 2, 3, 1.0),   # second s-tile: one sub-tile and one row
    (2, 63, 70, 128, 2, 0, 1.0),
    (2, 63, 70, 260, 2, 1, 1.0),    # Npad 272: three column tiles
    (2, 63, 65, 130, 2, 2, 1.0),
    (2, 63, 65, 130, 4, 1, 1.0),    # four images: the KC = 8 staging
    (2, 577, 3, 260, 4, 2, 1.0),    # KC = 8 with two chunks, general softmax
    (2, 63, 3, 130, 2, 3, 1.0),
    (2, 63, 65, 130, 2, 3, 0.7),    # ey0 is the weighted mean of sigma(-z)
]


@pytest.mark.parametrize("b,s,m,n,n_out,act,wsum", TILED_CASES)
def test_fused_predict_tiled_vs_fp64(ext, b, s, m, n, n_out, act, wsum):
    mpad = max(16, _ceil(m, 16))
    masks, diff, base, wbg = _operands(
        b, s, m, n, n_out, act, 4000 + s + m + n + act, mpad, wsum=wsum)
    ey = _run_tiled(ext, masks, diff, base, wbg, n_out, act)
    name = (f"fused_predict_tiled b={b} s={s} m={m} n={n} o={n_out} act={act} "
            f"wsum={wsum}")
    _check(name, ey, masks, diff, base, wbg, n, n_out, act, mpad)


def test_fused_predict_tiled_rejects_mpad_20(ext):
    masks = torch.ones(1, 4, 3, dtype=torch.uint8, device=DEV)
    diff = torch.zeros(1, 1, 20, 16, device=DEV)
    base = torch.zeros(1, 16, device=DEV)
    wbg = torch.zeros(16, device=DEV)
    with pytest.raises(RuntimeError, match=r"Mpad%16==0"):
        _run_tiled(ext, masks, diff, base, wbg, 1, 1)


# --------------------------------------------------------------------------- #
# fused_predict_tiled_bf16: bf16 MFMA per 32-deep k block

# (b, s, m, n, n_out, act, split, wsum)
TILED_BF16_CASES = [
    # double-buffered staging (split * images == 1)
    (2, 1, 3, 16, 1, 0, 1, 1.0),        # Mpad 32: one chunk
    (2, 63, 40, 128, 1, 1, 1, 1.0),     # Mpad 64: both ping-pong buffers
    (2, 577, 65, 130, 1, 1, 1, 1.0),    # Mpad 96: an odd chunk count
    (2, 577, 65, 130, 2, 3, 1, 1.0),
    (2, 63, 40, 260, 2, 3, 1, 1.0),
    (2, 63, 65, 130, 2, 3, 1, 0.7),
    # single-buffered staging
    (2, 63, 65, 130, 2, 3, 2, 1.0),     # split 2
    (2, 63, 3, 16, 1, 1, 2, 1.0),
    (2, 577, 40, 260, 2, 1, 1, 1.0),    # two images
    (2, 63, 65, 130, 2, 2, 2, 1.0),     # split * images == 4
    (2, 63, 65, 130, 4, 1, 1, 1.0),     # four images
    (2, 1, 40, 128, 4, 2, 1, 1.0),
    (2, 63, 65, 130, 2, 0, 1, 1.0),
]


@pytest.mark.parametrize("b,s,m,n,n_out,act,split,wsum", TILED_BF16_CASES)
def test_fused_predict_tiled_bf16_vs_fp64(ext, b, s, m, n, n_out, act, split,
                                          wsum):
    mpad = max(32, _ceil(m, 32))
    masks, diff, base, wbg = _operands(
        b, s, m, n, n_out, act, 5000 + s + m + n + act + split, mpad,
        wsum=wsum, bf16_headroom=True)
    diffb, deq = _bf16_images(diff, split, mpad)
    ey = _run_tiled(ext, masks, diffb, base, wbg, n_out, act, bf16=True)
    name = (f"fused_predict_tiled_bf16 b={b} s={s} m={m} n={n} o={n_out} "
            f"act={act} split={split} wsum={wsum}")
    _check_bf16(name, ey, masks, diff, deq, base, wbg, n, n_out, act, mpad,
                split)


def test_fused_predict_tiled_bf16_rejects_four_images_split_2(ext):
    masks = torch.ones(1, 4, 3, dtype=torch.uint8, device=DEV)
    diffb = torch.zeros(1, 2, 4, 16, 32, dtype=torch.bfloat16, device=DEV)
    base = torch.zeros(4, 16, device=DEV)
    wbg = torch.zeros(16, device=DEV)
    with pytest.raises(RuntimeError, match="LDS footprint"):
        _run_tiled(ext, masks, diffb, base, wbg, 4, 1, bf16=True)


# --------------------------------------------------------------------------- #
# saturated act 3 on the tiled kernels: p0 = p1 * exp(-z) keeps both outputs
# relatively accurate

@pytest.mark.parametrize("shift", [30.0, -30.0])
@pytest.mark.parametrize("kernel", ["tiled", "tiled_bf16_split1",
                                    "tiled_bf16_split2"])
def test_tiled_act3_saturated_relative(ext, kernel, shift):
    """|z - shift| <= 1 with shift = +-30: one of the two outputs is ~1e-13.
    Derived relative error: dz + |z| * log2(e) * 2^-23 + a few ulp ~ 5e-6 at
    |z| <= 31; the bound is the project's rtol for this epilogue, 1e-4, with
    no absolute floor."""
    b, s, m, n, n_out, act = 2, 63, 65, 130, 2, 3
    bf16 = kernel != "tiled"
    mpad = _ceil(m, 32) if bf16 else _ceil(m, 16)
    masks, diff, base, wbg = _operands(
        b, s, m, n, n_out, act, 6000, mpad, zscale=1.0, bf16_headroom=bf16)
    base[:, :n] += shift
    if bf16:
        operand, diff_ref = _bf16_images(diff, int(kernel[-1]), mpad)
    else:
        operand, diff_ref = diff, diff
    ey = _run_tiled(ext, masks, operand, base, wbg, n_out, act, bf16=bf16)
    z, _, ref = fp64_reference(masks, diff_ref, base, wbg, act)
    assert (z[..., :n] - shift).abs().max().item() <= 1.0 + 1e-6
    assert not bool(torch.isnan(ey).any())
    small = 0 if shift > 0 else 1
    assert ref[..., small].max().item() < 1e-12
    rel = ((ey.double() - ref).abs() / ref).amax(dim=(0, 1))
    print(f"{kernel} act 3 saturated shift={shift:+.0f}: max rel err "
          f"ey0={rel[0].item():.3e} ey1={rel[1].item():.3e} bound=1e-4")
    assert bool(((ey.double() - ref).abs() <= 1e-4 * ref).all())


# --------------------------------------------------------------------------- #
# determinism: two launches into fresh NaN-filled outputs, bit-identical

@pytest.mark.parametrize("kernel", ["linear", "bf16", "tiled", "tiled_bf16"])
def test_u8_predict_kernels_bitwise_deterministic(ext, kernel):
    b, s, n, n_out, act = 2, 577, 130, 2, 1
    if kernel in ("linear", "bf16"):
        n = 100
    m = {"linear": 40, "bf16": 30, "tiled": 65, "tiled_bf16": 65}[kernel]
    mpad = {"linear": 40, "bf16": 32, "tiled": 80, "tiled_bf16": 96}[kernel]
    masks, diff, base, wbg = _operands(b, s, m, n, n_out, act, 7000, mpad)
    if kernel == "linear":
        run = lambda: _run_linear(ext, masks, diff, base, wbg, n_out, act)
    elif kernel == "bf16":
        diffb, _ = _bf16_images(diff, 2, KSTRIDE_BF)
        run = lambda: _run_bf16(ext, masks, diffb, base, wbg, n_out, act)
    elif kernel == "tiled":
        run = lambda: _run_tiled(ext, masks, diff, base, wbg, n_out, act)
    else:
        diffb, _ = _bf16_images(diff, 2, mpad)
        run = lambda: _run_tiled(ext, masks, diffb, base, wbg, n_out, act,
                                 bf16=True)
    e1, e2 = run(), run()
    assert not bool(torch.isnan(e1).any())
    assert torch.equal(e1, e2)


# --------------------------------------------------------------------------- #
# the user-visible path: buckets the engine sends to these kernels

def _softmax4_engine(n_groups, dtype):
    from distributedkernelshap_amd.config import KernelConfig
    from distributedkernelshap_amd.core.engine import KernelShapEngine
    from distributedkernelshap_amd.models import LinearPredictor, make_tabular

    data = make_tabular(n_features=n_groups, n_instances=3, n_background=100,
                        seed=11)
    pred = LinearPredictor.random(n_groups, 4, seed=11, activation="softmax")
    eng = KernelShapEngine(
        pred, data.background, groups=data.groups, link="identity", seed=0,
        device="cuda", kernels=KernelConfig(predict_dtype=dtype),
    )
    calls = {}
    for meth in ("_ey_fused_linear", "_ey_fused_bf16"):
        def wrapped(*a, _orig=getattr(eng._gpu, meth), _meth=meth, **k):
            calls[_meth] = calls.get(_meth, 0) + 1
            return _orig(*a, **k)
        setattr(eng._gpu, meth, wrapped)
    return eng, data, calls


def test_engine_softmax4_40_groups_fp32_vs_fp64():
    """4-class softmax, 40 single-column groups, 100 background rows: the
    bucket runs fused_predict_linear with four images at Mpad 40, Npad 112
    (73,920 B of dynamic LDS)."""
    e32, data, calls = _softmax4_engine(40, "fp32")
    e64, _, _ = _softmax4_engine(40, "fp64")
    r32 = e32.shap_values(data.X, nsamples=600, l1_reg=False)
    assert set(calls) == {"_ey_fused_linear"}, calls
    r64 = e64.shap_values(data.X, nsamples=600, l1_reg=False)
    assert len(r32) == 4 and r32[0].shape == (3, 40)
    errs = [np.abs(r32[o] - r64[o]).max() for o in range(4)]
    print(f"engine softmax-4 m=40 fp32 vs fp64: max|dphi|={max(errs):.3e} "
          f"bound=1e-3")
    assert sum(np.abs(r64[o]).sum() for o in range(4)) > 0
    assert max(errs) < 1e-3


def test_engine_softmax4_30_groups_bf16x2_vs_fp32():
    """The same predictor family at m = 30 with predict_dtype bf16x2: the
    bucket runs fused_predict_bf16 with four hi + lo images at Npad 112
    (73,928 B of dynamic LDS)."""
    eb2, data, calls_b = _softmax4_engine(30, "bf16x2")
    e32, _, calls_f = _softmax4_engine(30, "fp32")
    rb2 = eb2.shap_values(data.X, nsamples=600, l1_reg=False)
    assert set(calls_b) == {"_ey_fused_bf16"}, calls_b
    r32 = e32.shap_values(data.X, nsamples=600, l1_reg=False)
    assert set(calls_f) == {"_ey_fused_linear"}, calls_f
    errs = [np.abs(rb2[o] - r32[o]).max() for o in range(4)]
    print(f"engine softmax-4 m=30 bf16x2 vs fp32: max|dphi|={max(errs):.3e} "
          f"bound=2e-3")
    assert sum(np.abs(r32[o]).sum() for o in range(4)) > 0
    assert max(errs) < 2e-3
