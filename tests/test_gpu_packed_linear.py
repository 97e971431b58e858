"""Packed linear pipeline: the four kernels that run the linear KernelSHAP
step from packed mask words (fill_masks_packed, linear_prepare,
fused_predict_linear_packed, wls_solve_packed), each against the kernel or
torch chain it replaces, plus the engine end to end."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

DEV = "cuda"


@pytest.fixture(scope="module")
def ext():
    from distributedkernelshap_amd.ops import load_extension

    return load_extension()


# ----------------------------------------------------------------------- #
# 1. sampler: bit-identical to enum copy -> fill_random_masks -> pack_masks

@pytest.mark.parametrize(
    "m,s,n_enum,n_rand",
    [(12, 130, 24, 106), (5, 20, 10, 10), (10, 1022, 1022, 0),
     (64, 200, None, None)],
)
def test_fill_masks_packed_equals_u8_path(ext, m, s, n_enum, n_rand):
    from distributedkernelshap_amd.core.sampler import plan_coalitions

    plan = plan_coalitions(m, s)
    ne = plan.enum_masks.shape[0]
    assert plan.nsamples == s
    if n_enum is not None:
        assert (ne, plan.n_random) == (n_enum, n_rand)
    else:
        assert plan.n_random > 0
    b = 3
    ids = torch.tensor([5, 1000, 7], dtype=torch.int32, device=DEV)
    cdf = torch.tensor(
        np.cumsum(plan.random_size_probs).astype(np.float32), device=DEV)
    szs = torch.tensor(plan.random_sizes.astype(np.int32), device=DEV)
    num_paired = int(np.floor((m - 1) / 2.0))
    if plan.n_random > 0 and m == 12:
        # both paired and unpaired draws are in play
        assert plan.random_sizes.min() <= num_paired < plan.random_sizes.max()
    enum = torch.tensor(plan.enum_masks, dtype=torch.uint8, device=DEV)

    masks = torch.zeros(b, s, m, dtype=torch.uint8, device=DEV)
    masks[:, :ne] = enum[None]
    if plan.n_random > 0:
        ext.fill_random_masks(
            masks, ne, plan.n_random, cdf, szs, num_paired, 3, ids)
    ref = torch.empty(b, s, dtype=torch.int64, device=DEV)
    ext.pack_masks(masks, ref)

    enum_packed = torch.empty(1, ne, dtype=torch.int64, device=DEV)
    if ne > 0:
        ext.pack_masks(enum[None].contiguous(), enum_packed)
    packed = torch.full((b, s), -1, dtype=torch.int64, device=DEV)
    ext.fill_masks_packed(
        packed, enum_packed[0].contiguous(), plan.n_random, cdf, szs,
        num_paired, 3, ids, m)
    assert torch.equal(packed, ref)
    if m == 64:
        # bit 63 is drawn, and complements carry it too
        assert bool((packed < 0).any())


# ----------------------------------------------------------------------- #
# 2./3. predict

def _predict_operands(b, s, m, n, n_out, act, seed, mask_p=0.5, zscale=None):
    g = torch.Generator(device=DEV).manual_seed(seed)
    oimg = 1 if act == 3 else n_out
    mpad = max(4, (m + 3) // 4 * 4)
    npad = (n + 15) // 16 * 16
    masks = (torch.rand(b, s, m, generator=g, device=DEV) > mask_p).to(torch.uint8)
    diff = torch.zeros(b, oimg, mpad, npad, device=DEV)
    diff[:, :, :m, :n] = torch.randn(b, oimg, m, n, generator=g, device=DEV)
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


PREDICT_CASES = (
    [(3, 200, 12, 100, n_out, act)
     for n_out in (1, 2) for act in (0, 1, 2, 3)
     if not (act == 3 and n_out != 2) and not (act == 2 and n_out == 1)]
    + [(2, 130, 10, 37, 2, 2),      # nothing a multiple of the tile sizes
       (1, 70, 17, 16, 2, 1),       # Mpad = 20: runtime k loop
       (1, 70, 17, 16, 2, 2),
       (1, 70, 64, 16, 2, 3),       # bit 63 is an A element
       (1, 70, 64, 16, 1, 1)]
)


@pytest.mark.parametrize("b,s,m,n,n_out,act", PREDICT_CASES)
def test_predict_packed_matches_u8_kernel(ext, b, s, m, n, n_out, act):
    masks, packed, diff, base, wbg = _predict_operands(
        b, s, m, n, n_out, act, seed=42 + m)
    ref = torch.empty(b, s, n_out, device=DEV)
    ext.fused_predict_linear(masks, diff, base, wbg, ref, act)
    ey = torch.full((b, s, n_out), float("nan"), device=DEV)
    ext.fused_predict_linear_packed(packed, diff, base, wbg, ey, act)
    err = (ey - ref).abs().max().item()
    print(f"packed vs u8 predict act={act} n_out={n_out} m={m}: max|d|={err:.3e}")
    assert torch.allclose(ey, ref, atol=2e-5, rtol=1e-4), err
    # identity link with lfnull: a plain subtraction
    lf = torch.linspace(-0.5, 0.5, n_out, device=DEV)
    ey2 = torch.empty_like(ey)
    ext.fused_predict_linear_packed(packed, diff, base, wbg, ey2, act, 0, lf)
    assert torch.allclose(ey2, ref - lf[None, None], atol=2e-5, rtol=1e-4)


@pytest.mark.parametrize("n_out,act", [(2, 3), (2, 1), (1, 1)])
def test_predict_packed_fused_logit_link(ext, n_out, act):
    b, s, m, n = 2, 200, 12, 100
    masks, packed, diff, base, wbg = _predict_operands(
        b, s, m, n, n_out, act, seed=5, zscale=6.0)
    lf = torch.tensor([0.3, -0.2][:n_out], device=DEV)
    ey = torch.empty(b, s, n_out, device=DEV)
    ext.fused_predict_linear_packed(packed, diff, base, wbg, ey, act, 1, lf)
    # fp64 evaluation of the same operands
    z = torch.einsum("bsk,bokn->bson", masks.double(), diff[:, :, :m].double())
    z = z + base.double()[None, None]
    assert z.abs().max().item() <= 6.0 + 1e-9
    if act == 3:
        p1 = torch.sigmoid(z[:, :, 0])
        pn = torch.stack([1.0 - p1, p1], dim=2)               # (b,s,2,n)
    else:
        pn = torch.sigmoid(z)
    p = torch.einsum("bson,n->bso", pn, wbg.double())
    ref = torch.log(p / (1.0 - p)) - lf.double()[None, None]
    # predict tolerance pushed through the logit's derivative 1/(p(1-p))
    tol = (2e-5 + 1e-4 * p) / (p * (1.0 - p))
    d = (ey.double() - ref).abs()
    print(f"fused link act={act} n_out={n_out}: max|d|={d.max().item():.3e} "
          f"max d/tol={(d / tol).max().item():.3e}")
    assert bool((d <= tol).all())


def test_predict_packed_fused_link_saturated(ext):
    """|z| ~ 40: every probability clamps; the fused link stays finite and
    equals the torch link chain applied to the unfused kernel's output."""
    # n = 64: the background weights 1/64 are exact, so a saturated row sums
    # to exactly 1
    b, s, m, n, n_out, act = 1, 130, 12, 64, 2, 1
    masks, packed, diff, base, wbg = _predict_operands(
        b, s, m, n, n_out, act, seed=6, zscale=1.0)
    base[0, :n] += 40.0
    base[1, :n] -= 40.0
    lf = torch.tensor([0.3, -0.2], device=DEV)
    ey = torch.empty(b, s, n_out, device=DEV)
    ext.fused_predict_linear_packed(packed, diff, base, wbg, ey, act, 1, lf)
    assert bool(torch.isfinite(ey).all())
    p = torch.empty(b, s, n_out, device=DEV)
    ext.fused_predict_linear(masks, diff, base, wbg, p, act)
    assert bool(((p < 1e-7) | (p > 1.0 - 1e-7)).all())     # all clamp
    p = p.clamp(1e-7, 1.0 - 1e-7)
    lp = torch.log(p)
    ref = lp - torch.log1p(-torch.exp(lp)) - lf[None, None]
    err = ((ey - ref).abs() / ref.abs()).max().item()
    print(f"saturated fused link: max rel d={err:.3e}")
    assert torch.allclose(ey, ref, rtol=1e-5, atol=0.0), err


# ----------------------------------------------------------------------- #
# 4. WLS

def test_wls_solve_packed_vs_cpu(ext):
    from distributedkernelshap_amd.core.solver import solve_wls

    g = torch.Generator(device=DEV).manual_seed(11)
    b, s, m, n_out, G = 5, 500, 12, 2, 14
    masks = (torch.rand(b, s, m, generator=g, device=DEV) > 0.5).to(torch.uint8)
    masks[:, :, 0] = (torch.rand(b, s, generator=g, device=DEV) > 0.3).to(torch.uint8)
    kw = torch.rand(s, generator=g, device=DEV) + 0.05
    ey = torch.randn(b, s, n_out, generator=g, device=DEV)
    total = torch.randn(b, n_out, generator=g, device=DEV)
    packed = torch.empty(b, s, dtype=torch.int64, device=DEV)
    ext.pack_masks(masks, packed)
    skipped = [3, 9]
    varying = [i for i in range(G) if i not in skipped]
    vidx = torch.tensor(varying, dtype=torch.int64, device=DEV)
    phi_full = torch.full((b, G, n_out), float("nan"), device=DEV)
    ext.wls_solve_packed(packed, kw, ey, total, vidx, phi_full)

    kwb = kw[None].expand(b, s).contiguous()
    phi_old = torch.empty(b, m, n_out, device=DEV)
    ext.wls_solve(masks, kwb, ey, total, phi_old, packed)
    print("wls packed vs broadcast-weight kernel: max|d|="
          f"{(phi_full[:, vidx] - phi_old).abs().max().item():.3e}")

    ph = phi_full.cpu().numpy()
    assert np.all(ph[:, skipped] == 0.0)
    for i in range(b):
        ref = solve_wls(
            masks[i].cpu().numpy(),
            kw.double().cpu().numpy(),
            ey[i].double().cpu().numpy(),
            total[i].double().cpu().numpy(),
        )
        got = ph[i][varying]
        assert np.allclose(got, ref, atol=5e-3, rtol=1e-3), np.abs(got - ref).max()
        assert np.allclose(ph[i].sum(axis=0), total[i].cpu().numpy(), atol=1e-4)


# ----------------------------------------------------------------------- #
# 5. linear_prepare

@pytest.mark.parametrize("act,link", [(1, 1), (3, 1), (2, 0), (0, 0)])
def test_linear_prepare(ext, act, link):
    g = torch.Generator(device=DEV).manual_seed(23)
    b, d, G, n, n_out = 4, 50, 12, 37, 2
    oimg = 1 if act == 3 else n_out
    X = torch.randn(b, d, generator=g, device=DEV)
    W = torch.randn(n_out, d, generator=g, device=DEV)
    bias = torch.randn(n_out, generator=g, device=DEV)
    col_group = torch.arange(d, device=DEV) % G           # every group populated
    col_group = col_group[torch.randperm(d, generator=g, device=DEV)].contiguous()
    varying = [0, 1, 2, 4, 5, 6, 7, 8, 10, 11]            # m = 10 -> Mpad 12
    m, mpad, npad = len(varying), 12, 48
    vidx = torch.tensor(varying, dtype=torch.int64, device=DEV)
    bgp = torch.randn(n, G, oimg, generator=g, device=DEV)
    lfnull64 = torch.tensor([0.4, -0.4], dtype=torch.float64, device=DEV)
    diff = torch.full((b, oimg, mpad, npad), float("nan"), device=DEV)
    total = torch.full((b, n_out), float("nan"), device=DEV)
    ext.linear_prepare(X, W, bias, col_group, vidx, bgp, lfnull64, diff,
                       total, act, link)

    # fp64 reference of the diff image
    contrib = X.double()[:, :, None] * W.double().T[None]            # (b,d,o)
    xp = torch.zeros(b, G, n_out, dtype=torch.float64, device=DEV)
    xp.index_add_(1, col_group, contrib)
    # D * 2^-23 * max_j |x_j W_oj| per (instance, output)
    bound = d * 2.0 ** -23 * contrib.abs().amax(dim=1)               # (b,o)
    if act == 3:
        xp = xp[:, :, 1:2] - xp[:, :, 0:1]
        bound = bound.sum(dim=1, keepdim=True)    # two images subtracted
    ref = (xp[:, vidx].permute(0, 2, 1)[:, :, :, None]
           - bgp.double()[:, vidx].permute(2, 1, 0)[None])           # (b,oi,m,n)
    err = (diff[:, :, :m, :n].double() - ref).abs()
    print(f"linear_prepare act={act}: diff max err={err.max().item():.3e} "
          f"min bound={bound.min().item():.3e}")
    assert bool((err <= bound[:, :, None, None]).all())
    assert bool((diff[:, :, m:, :] == 0).all())
    assert bool((diff[:, :, :, n:] == 0).all())

    # totals: the torch chain the engine runs
    z = X.double() @ W.double().T + bias.double()
    if act == 1:
        p = torch.sigmoid(z)
    elif act in (2, 3):
        p = torch.softmax(z, dim=-1)
    else:
        p = z
    if link:
        p = torch.clamp(p, 1e-15, 1.0 - 1e-15)
        p = torch.log(p / (1.0 - p))
    tref = (p - lfnull64[None]).float()
    assert torch.allclose(total, tref, rtol=1e-6, atol=2e-6), (
        (total - tref).abs().max().item())


# ----------------------------------------------------------------------- #
# 6. end to end

def _adult(seed):
    from distributedkernelshap_amd.models import LinearPredictor, make_adult_like

    data = make_adult_like(n_instances=8, n_background=100, seed=seed)
    return data, LinearPredictor.random(data.X.shape[1], 2, seed=seed)


def _engine(pred, bg, groups, dtype):
    from distributedkernelshap_amd.config import KernelConfig
    from distributedkernelshap_amd.core.engine import KernelShapEngine

    return KernelShapEngine(
        pred, bg, groups=groups, link="logit", seed=0, device="cuda",
        kernels=KernelConfig(predict_dtype=dtype),
    )


def test_engine_packed_eager_capture_replay_and_fp64():
    data, pred = _adult(12)
    e32 = _engine(pred, data.background, data.groups, "fp32")
    e64 = _engine(pred, data.background, data.groups, "fp64")
    X = data.X
    r1 = e32.shap_values(X)        # eager
    r2 = e32.shap_values(X)        # capture
    r3 = e32.shap_values(X)        # speculative replay
    gpu = e32._gpu
    assert any(k[0] == "packed" for k in gpu._enum_cache), (
        "the packed pipeline should have served this engine")
    for o in range(2):
        assert np.allclose(r1[o], r2[o], atol=1e-6)
        assert np.allclose(r1[o], r3[o], atol=1e-6)
    ref = e64.shap_values(X)
    errs = [np.abs(r1[o] - ref[o]).max() for o in range(2)]
    print(f"packed pipeline vs fp64 engine: max err={max(errs):.3e}")
    assert max(errs) < 1e-3


def test_engine_packed_group_equal_to_background():
    """One group equals the background for every instance: m = 11 and one
    scattered row of exact zeros."""
    data, pred = _adult(13)
    cols = np.asarray(data.groups[2])
    bg = data.background.copy()
    bg[:, cols] = bg[0, cols]                 # constant background columns
    X = data.X.copy()
    X[:, cols] = bg[0, cols]
    e32 = _engine(pred, bg, data.groups, "fp32")
    e64 = _engine(pred, bg, data.groups, "fp64")
    r = [e32.shap_values(X) for _ in range(3)]
    ref = e64.shap_values(X)
    for o in range(2):
        for rr in r:
            assert np.all(rr[o][:, 2] == 0.0)
            assert np.allclose(rr[o], r[0][o], atol=1e-6)
        assert np.abs(r[0][o] - ref[o]).max() < 1e-3
        assert np.abs(r[0][o]).sum() > 0
