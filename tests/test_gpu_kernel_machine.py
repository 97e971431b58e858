"""Fused kernel-machine predict (fused_predict_kernelmachine) on the GPU: the
kernel against an explicit blend fed to the numpy oracle, and the engine end
to end against the CPU oracle."""
import logging

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from distributedkernelshap_amd.models import KernelMachinePredictor  # noqa: E402
from distributedkernelshap_amd.ops import km_pack  # noqa: E402


@pytest.fixture(scope="module")
def ext():
    from distributedkernelshap_amd.ops import load_extension

    return load_extension()


# ----------------------------------------------------------------------- #
# kernel level

def _chunked_groups(d, m):
    cuts = np.linspace(0, d, m + 1).round().astype(int)
    return [list(range(cuts[i], cuts[i + 1])) for i in range(m)]


# support-vector tiles one wave covers per pass of its tile loop
W = 1

# (D, groups, N, S, B, V, kernel, n_out, act, extra constructor arguments) —
# each the smallest shape that breaks one assumption
SHAPES = {
    # V, M and N below one tile / one wave's share; S not a tile multiple
    1: (7, [[0], [1, 2], [3], [4, 5, 6]], 3, 70, 1, 5, "rbf", 1, "none", {}),
    # V spans tiles with a ragged last one; N not a multiple of the waves' chunks
    2: (9, _chunked_groups(9, 5), 19, 70, 1, 37, "rbf", 2, "softmax", {}),
    3: (9, _chunked_groups(9, 5), 19, 70, 1, 37, "poly", 2, "sigmoid",
        dict(degree=3, coef0=0.5)),
    # odd powers of negative bases
    4: (9, _chunked_groups(9, 5), 19, 70, 1, 37, "poly", 2, "none",
        dict(degree=1, coef0=-0.3)),
    5: (9, _chunked_groups(9, 5), 19, 70, 1, 37, "poly", 2, "none",
        dict(degree=5, coef0=-0.3)),
    # one tile past a full pass, two sample tiles, fewer rows than waves,
    # three k chunks, all eight outputs
    6: (33, [[j] for j in range(33)], 2, 130, 1, 16 * W + 1, "rbf", 8,
        "softmax", {}),
    # B = 3 with distinct x per instance: the batch stride
    7: (9, _chunked_groups(9, 5), 19, 70, 3, 37, "rbf", 2, "softmax", {}),
    # 72 groups of which 64 vary: the background must rule in the other 8
    8: (72, [[j] for j in range(72)], 5, 70, 2, 21, "rbf", 2, "softmax", {}),
    # almost every kernel value underflows
    9: (9, _chunked_groups(9, 5), 19, 70, 1, 37, "rbf", 2, "softmax",
        dict(gamma=50.0)),
    # many tiles, a long fixed-order sum
    10: (9, _chunked_groups(9, 5), 5, 40, 2, 600, "rbf", 2, "softmax", {}),
}


def _problem(shape_id):
    d, groups, n, s, b, v, kernel, n_out, act, extra = SHAPES[shape_id]
    rng = np.random.Generator(np.random.Philox(key=[109, shape_id]))
    extra = dict(extra)
    gamma = extra.pop("gamma", None)
    pred = KernelMachinePredictor.random(
        d, n_out, n_sv=v, kernel=kernel, seed=shape_id, activation=act, **extra)
    if gamma is not None:
        pred = KernelMachinePredictor(
            pred.support_vectors, pred.alpha, pred.intercept, kernel=kernel,
            gamma=gamma, activation=act)
    x = rng.normal(size=(b, d))
    bg = rng.normal(size=(n, d))
    wbg = rng.uniform(0.2, 1.0, size=n)          # non-uniform
    wbg /= wbg.sum()
    col_group = np.empty(d, dtype=np.int64)
    for gi, g in enumerate(groups):
        col_group[g] = gi
    vmap = np.arange(len(groups), dtype=np.int64)
    if shape_id == 8:
        vmap[64:] = -1        # x differs there, yet the background must rule
    m = int((vmap >= 0).sum())
    masks = (rng.uniform(size=(b, s, m)) < 0.5).astype(np.uint8)
    return dict(pred=pred, x=x, bg=bg, wbg=wbg, masks=masks,
                col_group=col_group, vmap=vmap, n_groups=len(groups))


def _reference(p):
    """Explicit (B, S, N, D) blend fed to the numpy oracle."""
    b, s, _ = p["masks"].shape
    n, d = p["bg"].shape
    colv = p["vmap"][p["col_group"]]                           # (D,)
    on = np.where(colv >= 0, p["masks"][:, :, np.maximum(colv, 0)], 0) != 0
    rows = np.where(on[:, :, None, :], p["x"][:, None, None, :],
                    p["bg"][None, None, :, :])
    pr = p["pred"](rows.reshape(-1, d)).reshape(b, s, n, -1)
    return np.einsum("bsno,n->bso", pr, p["wbg"])


_REF = {}


def _ref(shape_id):
    """Problem + reference, computed once and shared (never mutated)."""
    if shape_id not in _REF:
        p = _problem(shape_id)
        _REF[shape_id] = (p, _reference(p))
    return _REF[shape_id]


def _run_kernel(ext, p, pred=None, masks=None, vmap=None):
    dev = "cuda"
    pred = p["pred"] if pred is None else pred
    masks = p["masks"] if masks is None else masks
    vmap = p["vmap"] if vmap is None else vmap
    pack = km_pack.pack_machine(pred.kernel_machine_params(), p["col_group"],
                                p["n_groups"], dev)
    vidx = torch.from_numpy(np.flatnonzero(vmap >= 0)).to(dev)
    xparts = km_pack.group_parts(pack, torch.from_numpy(p["x"]).to(dev))
    bgparts = km_pack.group_parts(pack, torch.from_numpy(p["bg"]).to(dev))
    xp = km_pack.image(pack, xparts, vidx)
    bgpn = km_pack.image(pack, bgparts, vidx, negate=True)
    base = km_pack.base(pack, bgparts)
    wbg = torch.from_numpy(p["wbg"]).float().to(dev)
    b, s, _ = masks.shape
    ey = torch.full((b, s, pred.n_out), float("nan"), device=dev)
    km_pack.fused_predict(ext, pack, torch.from_numpy(masks).to(dev), xp, bgpn,
                          base, wbg, ey)
    torch.cuda.synchronize()
    return ey.double().cpu().numpy()


@pytest.mark.parametrize("shape_id", sorted(SHAPES))
def test_fused_km_vs_blend_reference(ext, shape_id):
    """The project's fused-predict bounds. The fp32 subtraction fold puts
    about 5e-7 of absolute error into gamma·pre at D = 64 (less here),
    ``__expf`` adds a few 1e-7 relative; with sum|alpha| = 4 that is about
    3e-6 in z, a factor of six inside the bound."""
    p, ref = _ref(shape_id)
    ey = _run_kernel(ext, p)
    assert ey.shape == ref.shape
    assert np.isfinite(ey).all()
    err = np.abs(ey - ref).max()
    print(f"shape {shape_id}: fp32 max abs err vs blend reference = {err:.3e}"
          f" (max |ref| {np.abs(ref).max():.3g})")
    assert np.allclose(ey, ref, atol=2e-5, rtol=1e-4), err


def test_fused_km_batch_rows_differ(ext):
    # shape 7 is only a batch-stride guard if the instances really differ
    p, ref = _ref(7)
    assert np.abs(ref[0] - ref[1]).max() > 1e-3
    assert np.abs(ref[1] - ref[2]).max() > 1e-3


def test_fused_km_nonvarying_groups_matter(ext):
    # shape 8 only guards the non-varying groups if treating them as varying
    # would change the answer
    p, ref = _ref(8)
    q = dict(p, vmap=np.arange(72, dtype=np.int64),
             masks=np.concatenate(
                 [p["masks"], np.ones(p["masks"].shape[:2] + (8,), np.uint8)],
                 axis=2))
    assert np.abs(_reference(q) - ref).max() > 1e-3


def test_fused_km_underflow_shape_really_underflows(ext):
    # shape 9 only guards the underflow if the kernel values are that small
    p, ref = _ref(9)
    k = p["pred"].kernel_values(p["bg"])
    assert np.median(k) < 1e-45              # below the smallest f32 subnormal
    assert np.isfinite(ref).all()


def test_fused_km_two_launches_identical(ext):
    for shape_id in (2, 10):
        p, _ = _ref(shape_id)
        assert np.array_equal(_run_kernel(ext, p), _run_kernel(ext, p))


def test_fused_km_outside_envelope_raises(ext):
    p, _ = _ref(2)
    many = KernelMachinePredictor.random(9, 2, n_sv=km_pack.MAX_SV + 1, seed=1)
    with pytest.raises(RuntimeError, match="envelope"):
        _run_kernel(ext, p, pred=many)
    wide = KernelMachinePredictor.random(9, 9, n_sv=37, seed=1)
    with pytest.raises(RuntimeError, match="envelope"):
        _run_kernel(ext, p, pred=wide)
    steep = KernelMachinePredictor.random(9, 2, n_sv=37, kernel="poly",
                                          degree=9, seed=1)
    with pytest.raises(RuntimeError, match="envelope"):
        _run_kernel(ext, p, pred=steep)
    # 65 varying groups
    q, _ = _ref(8)
    vmap = np.arange(72, dtype=np.int64)
    vmap[65:] = -1
    masks = np.concatenate(
        [q["masks"], np.ones(q["masks"].shape[:2] + (1,), np.uint8)], axis=2)
    with pytest.raises(RuntimeError, match="envelope"):
        _run_kernel(ext, q, masks=masks, vmap=vmap)


# ----------------------------------------------------------------------- #
# end to end: d = 8 singleton groups, full enumeration (no sampling noise)

D = 8


def _e2e_data():
    rng = np.random.Generator(np.random.Philox(key=[113, 8]))
    return rng.normal(size=(30, D)), rng.normal(size=(4, D))


def _engine(pred, bg, device, **kernel_kw):
    from distributedkernelshap_amd.config import KernelConfig
    from distributedkernelshap_amd.core.engine import KernelShapEngine

    return KernelShapEngine(
        pred, bg, link="logit", seed=0, device=device,
        kernels=KernelConfig(**kernel_kw) if kernel_kw else None,
    )


@pytest.fixture(scope="module")
def e2e():
    """Predictor, data, CPU-oracle values and one fused GPU engine."""
    pred = KernelMachinePredictor.random(D, 2, n_sv=40, kernel="rbf", seed=0,
                                         activation="softmax")
    bg, X = _e2e_data()
    sv_cpu = _engine(pred, bg, "cpu").shap_values(X)
    return pred, bg, X, sv_cpu, _engine(pred, bg, "cuda")


def test_engine_fused_km_matches_cpu_oracle(e2e):
    from distributedkernelshap_amd.core.links import logit

    pred, bg, X, sv_cpu, gpu = e2e
    assert gpu._gpu.km_fused is True
    sv = gpu.shap_values(X)
    fx = logit(pred(X))
    for o in range(2):
        assert sv[o].shape == (4, D)
        assert np.allclose(sv[o], sv_cpu[o], atol=5e-4, rtol=5e-3), \
            np.abs(sv[o] - sv_cpu[o]).max()
        total = sv[o].sum(axis=1) + gpu.expected_value[o]
        assert np.abs(total - fx[:, o]).max() < 1e-3


def test_engine_fused_km_deterministic_and_split(e2e):
    pred, bg, X, sv_cpu, gpu = e2e
    a = gpu.shap_values(X)
    b = gpu.shap_values(X)
    p1 = gpu.shap_values(X[:2], instance_offset=0)
    p2 = gpu.shap_values(X[2:], instance_offset=2)
    for o in range(2):
        assert np.array_equal(a[o], b[o])
        assert np.allclose(a[o], np.concatenate([p1[o], p2[o]]), atol=1e-5)


def test_fused_km_on_sample_slice(e2e):
    """The sample-sharded path hands the shared non-linear helper a slice of
    the sample axis: the slice's ey equals the same rows of the full call
    (a sample's arithmetic does not depend on its position in the tile)."""
    pred, bg, X, _, gpu = e2e
    g = gpu._gpu
    plan = gpu._plan(D, None)
    masks, _ = g._device_masks(plan, np.array([0]))
    X_dev = torch.tensor(X[:1], dtype=torch.float32, device="cuda")
    varying = np.arange(D)
    full = g._ey_predict_nonlinear(masks, X_dev, varying).clone()
    lo, hi = 37, 201              # neither a tile boundary
    assert hi < plan.nsamples
    part = g._ey_predict_nonlinear(masks[:, lo:hi], X_dev, varying)
    assert part.shape == (1, hi - lo, 2)
    assert torch.allclose(part, full[:, lo:hi], rtol=0.0, atol=1e-6)


def test_fused_km_bucket_split_along_b(e2e, monkeypatch):
    """A workspace budget that admits one instance per launch gives the same
    ey as one launch for the whole bucket."""
    pred, bg, X, _, gpu = e2e
    g = gpu._gpu
    plan = gpu._plan(D, None)
    masks, _ = g._device_masks(plan, np.arange(3))
    X_dev = torch.tensor(X[:3], dtype=torch.float32, device="cuda")
    varying = np.arange(D)
    whole = g.backend.ey_fused(masks, X_dev, varying).clone()
    monkeypatch.setattr(km_pack, "WORKSPACE_BYTES", 1)
    assert km_pack.instances_per_launch(g.backend.pack, D, D) == 1
    split = g.backend.ey_fused(masks, X_dev, varying)
    assert torch.equal(split, whole)


def test_engine_fused_km_mixed_buckets(e2e):
    pred, _, _, _, _ = e2e
    bg, X = _e2e_data()
    bg[:, 3] = 0.7                 # constant background column ...
    X[1, 3] = 0.7                  # ... that instance 1 matches: 7 varying
    sv_cpu = _engine(pred, bg, "cpu").shap_values(X)
    gpu = _engine(pred, bg, "cuda")
    sv = gpu.shap_values(X)
    assert gpu._gpu.km_fused is True
    for o in range(2):
        assert sv[o][1, 3] == 0.0
        assert np.allclose(sv[o], sv_cpu[o], atol=5e-4, rtol=5e-3), \
            np.abs(sv[o] - sv_cpu[o]).max()


def test_engine_too_many_support_vectors_falls_back_to_module_path(caplog):
    pred = KernelMachinePredictor.random(D, 2, n_sv=km_pack.MAX_SV + 1, seed=3)
    bg, X = _e2e_data()
    bg, X = bg[:10], X[:2]
    sv_cpu = _engine(pred, bg, "cpu").shap_values(X)
    with caplog.at_level(
            logging.INFO, logger="distributedkernelshap_amd.ops.gpu_engine"):
        gpu = _engine(pred, bg, "cuda")
        sv = gpu.shap_values(X)
        gpu.shap_values(X)
    assert gpu._gpu.km_fused is False
    reasons = [r for r in caplog.records
               if "fused kernel-machine kernel" in r.getMessage()]
    assert len(reasons) == 1
    assert f"{km_pack.MAX_SV + 1} support vectors" in reasons[0].getMessage()
    for o in range(2):
        assert np.allclose(sv[o], sv_cpu[o], atol=5e-4, rtol=5e-3), \
            np.abs(sv[o] - sv_cpu[o]).max()


def test_engine_km_fp64_mode_matches_cpu_oracle(e2e):
    pred, bg, X, sv_cpu, _ = e2e
    gpu = _engine(pred, bg, "cuda", predict_dtype="fp64")
    sv = gpu.shap_values(X)
    for o in range(2):
        assert np.allclose(sv[o], sv_cpu[o], rtol=0.0, atol=1e-8), \
            np.abs(sv[o] - sv_cpu[o]).max()


def test_engine_km_bf16_raises(e2e):
    pred, bg, _, _, _ = e2e
    with pytest.raises(ValueError, match="fp32"):
        _engine(pred, bg, "cuda", predict_dtype="bf16")
    with pytest.raises(ValueError, match="fp32"):
        _engine(pred, bg, "cuda", predict_dtype="bf16x2")


def test_engine_km_module_autocast_bf16_raises(e2e):
    pred, bg, _, _, _ = e2e
    with pytest.raises(ValueError, match="module_autocast"):
        _engine(pred, bg, "cuda", module_autocast="bf16")


def test_engine_leaves_the_predictor_untouched_and_picklable():
    import pickle

    pred = KernelMachinePredictor.random(D, 2, n_sv=12, seed=11)
    bg, X = _e2e_data()
    _engine(pred, bg, "cuda").shap_values(X[:1])
    assert pred._module is None
    clone = pickle.loads(pickle.dumps(pred))
    assert np.array_equal(clone(X), pred(X))


def test_kernel_shap_public_api_sklearn_svc():
    from sklearn.svm import SVC

    from distributedkernelshap_amd import KernelShap
    from distributedkernelshap_amd.models import make_adult_like

    data = make_adult_like(n_instances=8, n_background=25)
    train = make_adult_like(n_instances=200, n_background=1, seed=3).X
    y = (train[:, 0] + train[:, 1] * train[:, 2] > np.median(train[:, 0])).astype(int)
    est = SVC(kernel="rbf", gamma="scale").fit(train, y)
    pred = KernelMachinePredictor.from_sklearn(est)
    ks = KernelShap(pred, link="identity", device="cuda")
    ks.fit(data.background, groups=data.groups, group_names=data.group_names)
    assert ks._explainer._engine._gpu.km_fused is True
    exp = ks.explain(data.X)
    sv = exp.shap_values
    assert len(sv) == 1
    assert sv[0].shape == (8, 12)
    assert np.isfinite(sv[0]).all()
