"""fused_predict_linear_wide (3..16 outputs, column-tile-streamed image),
called directly and held to a float64 evaluation of the same operands.

Tolerance (tests/linear_predict_reference.py), computed per case from the
operands and never from what the kernel returns, with K_terms = Mpad:

    dz  = (Mpad + 1) * 2^-24 * max_col(|base| + sum_k |diff_k|)
    tol = L * dz + (N + 4) * 2^-24 * sum|w| * max|act| + 1e-6

L = 1 (identity), 1/4 (sigmoid), 1/2 (softmax). The kernel adds the column
tiles of one output in ascending order after a 16-lane reduction, which the
(N + 4) weighted adds of the reduction term cover. Every case prints its
measured error beside the tolerance.

The kernel predicates the pad classes out (their images are never read), so
the pad-class check is the bit-for-bit one: garbage in the pad images of diff
and base must not change a single output bit.
"""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from linear_predict_reference import (  # noqa: E402
    ZSCALE, column_bound, derived_tolerance, fp64_reference,
)

DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module")
def ext():
    from distributedkernelshap_amd.ops import load_extension

    return load_extension()


def _ceil(x, q):
    return (x + q - 1) // q * q


def _operands(b, s, m, n, n_out, act, seed, zscale=ZSCALE):
    """Random 0/1 masks (different per instance), a randn diff image
    (B, NOUTP, Mpad, Npad) with zero pad slots and zero pad images, a randn
    base (NOUTP, Npad) and non-uniform weights that sum to 1. For the
    probability activations |base| + sum_k |diff_k| <= zscale per column."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    noutp, mpad, npad = _ceil(n_out, 4), max(4, _ceil(m, 4)), _ceil(n, 16)
    masks = (torch.rand(b, s, m, generator=g, device=DEV) > 0.5).to(torch.uint8)
    diff = torch.zeros(b, noutp, mpad, npad, device=DEV)
    diff[:, :n_out, :m, :n] = torch.randn(b, n_out, m, n, generator=g,
                                          device=DEV)
    base = torch.zeros(noutp, npad, device=DEV)
    base[:n_out, :n] = torch.randn(n_out, n, generator=g, device=DEV)
    if act != 0:
        f = zscale / column_bound(diff, base) * (1.0 - 2.0 ** -20)
        diff *= f
        base *= f
    w = torch.rand(n, generator=g, device=DEV, dtype=torch.float64) + 0.1
    wbg = torch.zeros(npad, device=DEV)
    wbg[:n] = (w / w.sum()).float()
    return masks, diff, base, wbg


def _run(ext, masks, diff, base, wbg, n_out, act):
    b, s, _ = masks.shape
    ey = torch.full((b, s, n_out), NAN, device=DEV)
    ext.fused_predict_linear_wide(masks, diff, base, wbg, ey, act)
    return ey


def _check(name, ey, masks, diff, base, wbg, n, n_out, act, zmax=ZSCALE):
    """ey against the float64 evaluation of the n_out real images at the
    derived tolerance. Returns measured / tolerance."""
    mpad = diff.shape[2]
    dr, br = diff[:, :n_out], base[:n_out]
    z, p, ref = fp64_reference(masks, dr, br, wbg, act)
    if act != 0:
        assert z.abs().max().item() <= zmax + 1e-9
    assert not bool(torch.isnan(ey).any()), f"{name}: NaN left in ey"
    assert bool(torch.isfinite(ey).all()), f"{name}: inf in ey"
    tol = derived_tolerance(dr, br, wbg, p, n, n_out, act, mpad)
    err = (ey.double() - ref).abs().max().item()
    print(f"{name}: max|ey-fp64|={err:.3e} tol={tol:.3e} ratio={err / tol:.3f}")
    assert err <= tol, (name, err, tol)
    return err / tol


# (b, s, m, n, n_out, act)
CASES = [
    (2, 7, 2, 1, 3, 2),         # less than one MFMA tile; Mpad 4; one column
    (2, 7, 5, 100, 4, 2),       # top of width 4
    (2, 70, 5, 17, 5, 2),       # one class past width 4; Mpad 8; second tile
    (2, 70, 12, 100, 5, 0),
    (2, 600, 64, 100, 8, 0),    # top of width 8; Mpad 64; second s-tile
    (2, 70, 5, 512, 9, 1),      # one class past width 8; 32 column tiles
    (2, 600, 12, 100, 10, 2),   # the 10-class softmax the engine sends
    (2, 513, 12, 37, 10, 1),    # a second s-tile of one row
    (2, 70, 12, 17, 12, 1),     # top of width 12
    (2, 70, 12, 100, 13, 2),    # one class past width 12
    (2, 70, 64, 300, 16, 2),    # 64 KiB slice; Npad 304 > one-tile kernels
    (2, 600, 2, 300, 16, 0),
    (2, 70, 64, 512, 3, 2),     # every k slot and every column tile used
]


@pytest.mark.parametrize("b,s,m,n,n_out,act", CASES)
def test_fused_predict_linear_wide_vs_fp64(ext, b, s, m, n, n_out, act):
    masks, diff, base, wbg = _operands(
        b, s, m, n, n_out, act, 8000 + s + m + n + n_out + act)
    assert not torch.equal(masks[0], masks[1])
    assert not torch.equal(diff[0], diff[1])
    ey = _run(ext, masks, diff, base, wbg, n_out, act)
    name = (f"fused_predict_linear_wide b={b} s={s} m={m} n={n} o={n_out} "
            f"act={act}")
    _check(name, ey, masks, diff, base, wbg, n, n_out, act)


@pytest.mark.parametrize("s,n_out", [(70, 5), (600, 10), (7, 16)])
def test_wide_writes_exactly_b_s_nout(ext, s, n_out):
    """ey sits inside a larger NaN-filled buffer: no NaN is left inside
    (B, S, n_out), every element outside keeps the sentinel's bits."""
    b, m, n, act, guard = 2, 12, 100, 2, 4096
    masks, diff, base, wbg = _operands(b, s, m, n, n_out, act, 8100 + s)
    numel = b * s * n_out
    buf = torch.full((numel + 2 * guard,), NAN, device=DEV)
    sentinel = buf[:1].view(torch.int32).clone()
    ey = buf[guard:guard + numel].view(b, s, n_out)
    ext.fused_predict_linear_wide(masks, diff, base, wbg, ey, act)
    assert not bool(torch.isnan(ey).any())
    bits = buf.view(torch.int32)
    assert bool((bits[:guard] == sentinel).all())
    assert bool((bits[guard + numel:] == sentinel).all())
    _check(f"written region s={s} o={n_out}", ey, masks, diff, base, wbg, n,
           n_out, act)


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("n_out", [5, 9])
def test_wide_pad_classes_cannot_reach_an_output(ext, n_out, act):
    """Bit-identical output after the pad images of diff and base are
    overwritten with finite garbage."""
    b, s, m, n = 2, 200, 13, 100
    masks, diff, base, wbg = _operands(b, s, m, n, n_out, act, 8200 + n_out)
    clean = _run(ext, masks, diff, base, wbg, n_out, act)
    g = torch.Generator(device=DEV).manual_seed(8201)
    noutp = diff.shape[1]
    assert noutp > n_out
    diff[:, n_out:] = 1e3 * torch.randn(
        diff[:, n_out:].shape, generator=g, device=DEV)
    base[n_out:] = 1e30 * torch.randn(
        base[n_out:].shape, generator=g, device=DEV)
    dirty = _run(ext, masks, diff, base, wbg, n_out, act)
    assert not bool(torch.isnan(dirty).any())
    assert torch.equal(clean, dirty)
    _check(f"pad classes o={n_out} act={act}", dirty, masks, diff, base, wbg,
           n, n_out, act)


@pytest.mark.parametrize("n_out,lead", [(10, 9), (10, 0), (3, 1)])
def test_wide_saturated_softmax(ext, n_out, lead):
    """|z| <= 10 before one class is shifted up by 60: it leads by 40 to 80
    and the column bound reaches ~70. No NaN or inf, and the error stays
    within the derived tolerance, which scales with the column bound."""
    b, s, m, n, act = 2, 70, 12, 100, 2
    masks, diff, base, wbg = _operands(b, s, m, n, n_out, act, 8300 + lead,
                                       zscale=10.0)
    base[lead, :n] += 60.0
    cb = column_bound(diff[:, :n_out], base[:n_out])
    assert 50.0 <= cb <= 70.0 + 1e-3
    ey = _run(ext, masks, diff, base, wbg, n_out, act)
    z, _, _ = fp64_reference(masks, diff[:, :n_out], base[:n_out], wbg, act)
    others = [o for o in range(n_out) if o != lead]
    gap = (z[:, :, lead, :n].unsqueeze(2) - z[:, :, others, :n]).min().item()
    assert gap >= 40.0 - 1e-3
    _check(f"saturated softmax o={n_out} lead={lead} column_bound={cb:.1f}",
           ey, masks, diff, base, wbg, n, n_out, act, zmax=80.0)


def test_wide_bitwise_deterministic(ext):
    b, s, m, n, n_out, act = 2, 600, 40, 300, 10, 2
    masks, diff, base, wbg = _operands(b, s, m, n, n_out, act, 8400)
    e1 = _run(ext, masks, diff, base, wbg, n_out, act)
    e2 = _run(ext, masks, diff, base, wbg, n_out, act)
    assert not bool(torch.isnan(e1).any())
    assert torch.equal(e1, e2)


# (n_out, diff images, Mpad, Npad)
REFUSED = [
    (2, 4, 4, 16),          # fewer than 3 outputs
    (17, 20, 4, 16),        # more than 16 outputs
    (3, 4, 68, 16),         # Mpad 68
    (3, 4, 4, 528),         # Npad 528
    (3, 4, 4, 20),          # Npad 20: no multiple of 16
]


@pytest.mark.parametrize("n_out,noutp,mpad,npad", REFUSED)
def test_wide_refuses_outside_the_envelope(ext, n_out, noutp, mpad, npad):
    masks = torch.ones(1, 4, 3, dtype=torch.uint8, device=DEV)
    diff = torch.zeros(1, noutp, mpad, npad, device=DEV)
    base = torch.zeros(noutp, npad, device=DEV)
    wbg = torch.zeros(npad, device=DEV)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        _run(ext, masks, diff, base, wbg, n_out, 2)
