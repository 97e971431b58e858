"""Split-operand bf16 path of fused_predict_linear_packed (mma=1) against the
fp32-MFMA path (mma=0) on the same operands, each against an fp64 evaluation,
and the engine with KernelConfig(packed_mma="split") against "f32".

Bound between the two paths at zscale = 6 (|base| + sum_k |diff_k| <= 6 per
column): at most 13 fp32 additions of partial sums bounded by 6 give
<= 13 * 6 * 2^-24 = 4.7e-6 in z per path; the sigmoid's slope <= 1/4 turns
that into 1.2e-6 in p per path; two paths plus the shared epilogue's ~1e-7
round up to 4e-6.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

DEV = "cuda"
PATH_BOUND = 4e-6


@pytest.fixture(scope="module")
def ext():
    from distributedkernelshap_amd.ops import load_extension

    return load_extension()


def _predict_operands(b, s, m, n, n_out, act, seed, mask_p=0.5, zscale=None,
                      magnitudes=False):
    g = torch.Generator(device=DEV).manual_seed(seed)
    oimg = 1 if act == 3 else n_out
    mpad = max(4, (m + 3) // 4 * 4)
    npad = (n + 15) // 16 * 16
    masks = (torch.rand(b, s, m, generator=g, device=DEV) > mask_p).to(torch.uint8)
    diff = torch.zeros(b, oimg, mpad, npad, device=DEV)
    diff[:, :, :m, :n] = torch.randn(b, oimg, m, n, generator=g, device=DEV)
    if magnitudes:
        # entries randn * 10^U(-6, 1): mid and lo at very different exponents
        expo = torch.rand(b, oimg, m, n, generator=g, device=DEV) * 7.0 - 6.0
        diff[:, :, :m, :n] *= 10.0 ** expo
    base = torch.zeros(oimg, npad, device=DEV)
    base[:, :n] = torch.randn(oimg, n, generator=g, device=DEV)
    if zscale is not None:
        # |base| + sum_k |diff_k| <= zscale for every column
        bound = base.abs()[None] + diff.abs().sum(dim=2)
        f = zscale / bound.max()
        diff *= f
        base *= f
    wbg = torch.zeros(npad, device=DEV)
    wbg[:n] = 1.0 / n
    packed = torch.empty(b, s, dtype=torch.int64, device=DEV)
    from distributedkernelshap_amd.ops import load_extension

    load_extension().pack_masks(masks, packed)
    return masks, packed, diff, base, wbg


def _fp64_probabilities(masks, diff, base, wbg, m, act):
    z = torch.einsum("bsk,bokn->bson", masks.double(), diff[:, :, :m].double())
    z = z + base.double()[None, None]
    if act == 3:
        p1 = torch.sigmoid(z[:, :, 0])
        pn = torch.stack([1.0 - p1, p1], dim=2)               # (b,s,2,n)
    else:
        pn = torch.sigmoid(z)
    return z, torch.einsum("bson,n->bso", pn, wbg.double())


def _run(ext, packed, diff, base, wbg, shape, act, mma, link=0, lf=None):
    ey = torch.full(shape, float("nan"), device=DEV)
    ext.fused_predict_linear_packed(packed, diff, base, wbg, ey, act, link, lf,
                                    mma)
    return ey


# (b, s, m, n, n_out, act)
SPLIT_CASES = [
    (2, 200, 12, 100, 2, 3),    # the benchmark's tile shape
    (1, 530, 12, 100, 2, 3),    # two s-tiles, the second with 18 rows
    (2, 70, 1, 16, 1, 1),       # Mpad 4, NT 1
    (2, 130, 5, 37, 2, 1),      # Mpad 8, two images, N not a tile multiple
    (1, 70, 12, 128, 2, 3),     # NT 8
    (1, 70, 13, 16, 2, 3),      # Mpad 16: mma=1 falls back to the fp32 MFMA
]


@pytest.mark.parametrize("b,s,m,n,n_out,act", SPLIT_CASES)
def test_split_matches_f32_mfma_and_fp64(ext, b, s, m, n, n_out, act):
    masks, packed, diff, base, wbg = _predict_operands(
        b, s, m, n, n_out, act, seed=100 + m + n, zscale=6.0)
    shape = (b, s, n_out)
    e0 = _run(ext, packed, diff, base, wbg, shape, act, 0)
    e1 = _run(ext, packed, diff, base, wbg, shape, act, 1)
    ea = _run(ext, packed, diff, base, wbg, shape, act, -1)
    d = (e1 - e0).abs().max().item()
    z, ref = _fp64_probabilities(masks, diff, base, wbg, m, act)
    assert z.abs().max().item() <= 6.0 + 1e-9
    err0 = (e0.double() - ref).abs().max().item()
    err1 = (e1.double() - ref).abs().max().item()
    print(f"split vs f32 m={m} n={n} act={act}: max|d|={d:.3e} "
          f"vs fp64: f32 {err0:.3e} split {err1:.3e}")
    if m > 12:
        assert torch.equal(e1, e0)          # ineligible: the same kernel
    else:
        assert d <= PATH_BOUND, d
    assert torch.equal(ea, e1)              # auto = split where eligible
    for e in (e0, e1):
        assert torch.allclose(e.double(), ref, atol=2e-5, rtol=1e-4)


@pytest.mark.parametrize("n,falls_back", [(80, False), (128, True)])
def test_split_four_images(ext, n, falls_back):
    """Four operand images: 20 accumulator tiles run the two-half column
    split with the fragments read from LDS per sub-tile; 32 tiles of
    fragments do not fit the LDS and keep the fp32 MFMA."""
    b, s, m, n_out, act = 1, 70, 12, 4, 1
    masks, packed, diff, base, wbg = _predict_operands(
        b, s, m, n, n_out, act, seed=77, zscale=6.0)
    shape = (b, s, n_out)
    e0 = _run(ext, packed, diff, base, wbg, shape, act, 0)
    e1 = _run(ext, packed, diff, base, wbg, shape, act, 1)
    _, ref = _fp64_probabilities(masks, diff, base, wbg, m, act)
    d = (e1 - e0).abs().max().item()
    print(f"split four images n={n}: max|d|={d:.3e}")
    if falls_back:
        assert torch.equal(e1, e0)
    else:
        assert d <= PATH_BOUND, d
    assert torch.allclose(e1.double(), ref, atol=2e-5, rtol=1e-4)


@pytest.mark.parametrize("n_out,act", [(2, 3), (2, 1), (1, 1)])
def test_split_fused_logit_link(ext, n_out, act):
    b, s, m, n = 2, 200, 12, 100
    masks, packed, diff, base, wbg = _predict_operands(
        b, s, m, n, n_out, act, seed=5, zscale=6.0)
    lf = torch.tensor([0.3, -0.2][:n_out], device=DEV)
    ey = _run(ext, packed, diff, base, wbg, (b, s, n_out), act, 1, 1, lf)
    z, p = _fp64_probabilities(masks, diff, base, wbg, m, act)
    assert z.abs().max().item() <= 6.0 + 1e-9
    ref = torch.log(p / (1.0 - p)) - lf.double()[None, None]
    # predict tolerance pushed through the logit's derivative 1/(p(1-p))
    tol = (2e-5 + 1e-4 * p) / (p * (1.0 - p))
    d = (ey.double() - ref).abs()
    print(f"split fused link act={act} n_out={n_out}: max|d|={d.max().item():.3e} "
          f"max d/tol={(d / tol).max().item():.3e}")
    assert bool((d <= tol).all())


def test_split_fused_link_saturated(ext):
    """|z| ~ 40: every probability clamps; the fused link stays finite and
    equals the torch link chain applied to the unfused u8 kernel's output."""
    # n = 64: the background weights 1/64 are exact, so a saturated row sums
    # to exactly 1
    b, s, m, n, n_out, act = 1, 130, 12, 64, 2, 1
    masks, packed, diff, base, wbg = _predict_operands(
        b, s, m, n, n_out, act, seed=6, zscale=1.0)
    base[0, :n] += 40.0
    base[1, :n] -= 40.0
    lf = torch.tensor([0.3, -0.2], device=DEV)
    ey = _run(ext, packed, diff, base, wbg, (b, s, n_out), act, 1, 1, lf)
    assert bool(torch.isfinite(ey).all())
    p = torch.empty(b, s, n_out, device=DEV)
    ext.fused_predict_linear(masks, diff, base, wbg, p, act)
    assert bool(((p < 1e-7) | (p > 1.0 - 1e-7)).all())     # all clamp
    p = p.clamp(1e-7, 1.0 - 1e-7)
    lp = torch.log(p)
    ref = lp - torch.log1p(-torch.exp(lp)) - lf[None, None]
    err = ((ey - ref).abs() / ref.abs()).max().item()
    print(f"split saturated fused link: max rel d={err:.3e}")
    assert torch.allclose(ey, ref, rtol=1e-5, atol=0.0), err


@pytest.mark.parametrize("act,n_out", [(3, 2), (1, 2)])
def test_split_magnitudes(ext, act, n_out):
    """Diff entries spread over seven decades: the pieces of different
    entries sit at very different exponents."""
    b, s, m, n = 2, 200, 12, 100
    masks, packed, diff, base, wbg = _predict_operands(
        b, s, m, n, n_out, act, seed=31, zscale=6.0, magnitudes=True)
    nz = diff[:, :, :m, :n].abs()
    assert (nz.max() / nz[nz > 0].min()).item() > 1e6
    shape = (b, s, n_out)
    e0 = _run(ext, packed, diff, base, wbg, shape, act, 0)
    e1 = _run(ext, packed, diff, base, wbg, shape, act, 1)
    _, ref = _fp64_probabilities(masks, diff, base, wbg, m, act)
    d = (e1 - e0).abs().max().item()
    print(f"split magnitudes act={act}: max|d|={d:.3e} split vs fp64 "
          f"{(e1.double() - ref).abs().max().item():.3e}")
    assert d <= PATH_BOUND, d
    assert torch.allclose(e1.double(), ref, atol=2e-5, rtol=1e-4)


def test_split_group_equal_to_background(ext):
    """One diff row all zero (a group that equals the background)."""
    b, s, m, n, n_out, act = 2, 200, 12, 100, 2, 3
    masks, packed, diff, base, wbg = _predict_operands(
        b, s, m, n, n_out, act, seed=17, zscale=6.0)
    diff[:, :, 4] = 0.0
    shape = (b, s, n_out)
    e0 = _run(ext, packed, diff, base, wbg, shape, act, 0)
    e1 = _run(ext, packed, diff, base, wbg, shape, act, 1)
    _, ref = _fp64_probabilities(masks, diff, base, wbg, m, act)
    assert (e1 - e0).abs().max().item() <= PATH_BOUND
    assert torch.allclose(e1.double(), ref, atol=2e-5, rtol=1e-4)
    # the zero row's bit does not matter: clear it in every word
    cleared = packed & ~torch.tensor(1 << 4, dtype=torch.int64, device=DEV)
    e1c = _run(ext, cleared, diff, base, wbg, shape, act, 1)
    assert torch.equal(e1c, e1)


def test_engine_split_against_f32_eager_capture_replay():
    from distributedkernelshap_amd.config import KernelConfig
    from distributedkernelshap_amd.core.engine import KernelShapEngine
    from distributedkernelshap_amd.models import LinearPredictor, make_adult_like

    data = make_adult_like(n_instances=8, n_background=25, seed=21)
    pred = LinearPredictor.random(data.X.shape[1], 2, seed=21)

    def engine(mode):
        return KernelShapEngine(
            pred, data.background, groups=data.groups, link="logit", seed=0,
            device="cuda", kernels=KernelConfig(packed_mma=mode),
        )

    es, ef = engine("split"), engine("f32")
    X = data.X
    rf = ef.shap_values(X)
    total = ef.link(np.asarray(pred(X))) - ef.link(ef.fnull)[None, :]
    for call in ("eager", "capture", "replay"):
        rs = es.shap_values(X)
        for o in range(2):
            d = np.abs(rs[o] - rf[o]).max()
            t = np.abs(rs[o].sum(axis=1) - total[:, o]).max()
            print(f"engine split vs f32, {call}, class {o}: max|dphi|={d:.3e} "
                  f"max|sum-total|={t:.3e}")
            assert d <= 1e-5
            assert t <= 1e-4
    assert any(k[0] == "packed" for k in es._gpu._enum_cache), (
        "the packed pipeline should have served this engine")
    with pytest.raises(ValueError):
        engine("bf16").shap_values(X)
