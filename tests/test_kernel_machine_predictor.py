"""KernelMachinePredictor on the CPU: the oracle against a naive loop,
agreement with sklearn (SVC / NuSVC / SVR / NuSVR / KernelRidge), the torch
module, the fold identity of the fused kernel's operand images, and the
registry / loader wiring."""
import pickle

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from distributedkernelshap_amd.models import (  # noqa: E402
    KernelMachinePredictor,
    make_predictor,
)
from distributedkernelshap_amd.ops import km_pack  # noqa: E402

D = 6


def _data():
    rng = np.random.Generator(np.random.Philox(key=[83, 0]))
    X = rng.normal(size=(240, D))
    score = X[:, 0] + 0.5 * X[:, 1] * X[:, 2] - X[:, 3]
    return X, (score > 0).astype(int), score


def _fit(kind):
    pytest.importorskip("sklearn")
    from sklearn.kernel_ridge import KernelRidge
    from sklearn.svm import SVC, SVR, NuSVC, NuSVR

    X, y, score = _data()
    if kind == "svc_rbf":
        return SVC(kernel="rbf", gamma="scale").fit(X, y)
    if kind == "svc_poly":
        return SVC(kernel="poly", degree=3, coef0=0.5, gamma=0.2).fit(X, y)
    if kind == "nusvc":
        return NuSVC(kernel="rbf", gamma="auto", nu=0.4).fit(X, y)
    if kind == "svr":
        return SVR(kernel="rbf", gamma=0.3).fit(X, score)
    if kind == "nusvr":
        return NuSVR(kernel="poly", degree=2, coef0=1.0, gamma="scale").fit(X, score)
    if kind == "kr2":
        return KernelRidge(kernel="rbf", alpha=0.5).fit(
            X, np.stack([score, np.sin(score)], axis=1))
    if kind == "kr_poly":
        return KernelRidge(kernel="polynomial", degree=2, coef0=1.0,
                           gamma=0.1).fit(X, score)
    if kind == "svc_proba":
        # C = 10: a Platt fit whose 0.5 crossing lies within 0.1 of f = 0
        # (see the proba test)
        return SVC(kernel="rbf", gamma=0.2, C=10.0, probability=True,
                   random_state=0).fit(X, y)
    raise KeyError(kind)


_CASES = {}


def _case(kind):
    """Estimator, probe rows and wrapped predictor, built once per kind."""
    if kind not in _CASES:
        est = _fit(kind)
        rng = np.random.Generator(np.random.Philox(key=[89, 1]))
        rows = np.vstack([_data()[0][:40], rng.normal(size=(40, D))])
        _CASES[kind] = (est, rows, KernelMachinePredictor.from_sklearn(est))
    return _CASES[kind]


# ----------------------------------------------------------------------- #
# oracle

@pytest.mark.parametrize("kernel", ["rbf", "poly"])
@pytest.mark.parametrize("act", ["none", "sigmoid", "softmax"])
def test_oracle_matches_naive_loop(kernel, act):
    pred = KernelMachinePredictor.random(5, 3, n_sv=19, kernel=kernel, seed=2,
                                         activation=act, coef0=0.5, degree=3)
    rng = np.random.Generator(np.random.Philox(key=[97, 0]))
    X = rng.normal(size=(23, 5))
    want = np.empty((23, 3))
    for i in range(23):
        z = pred.intercept.copy()
        for v in range(19):
            sv = pred.support_vectors[v]
            if kernel == "rbf":
                k = np.exp(-pred.gamma * sum((X[i, j] - sv[j]) ** 2 for j in range(5)))
            else:
                k = (pred.gamma * sum(X[i, j] * sv[j] for j in range(5)) + 0.5) ** 3
            z += pred.alpha[:, v] * k
        if act == "softmax":
            e = np.exp(z - z.max())
            z = e / e.sum()
        elif act == "sigmoid":
            z = 1.0 / (1.0 + np.exp(-z))
        want[i] = z
    assert np.allclose(pred(X), want, rtol=0.0, atol=1e-13)


def test_oracle_chunks_over_rows():
    # more rows than one chunk of the (rows, V, D) difference tensor
    pred = KernelMachinePredictor.random(64, 2, n_sv=512, seed=3)
    rng = np.random.Generator(np.random.Philox(key=[97, 1]))
    X = rng.normal(size=(300, 64))
    assert (1 << 22) // (512 * 64) < 300
    full = pred(X)
    assert np.array_equal(full[290:], pred(X[290:]))


def test_random_is_seeded_and_scaled():
    a = KernelMachinePredictor.random(7, 3, n_sv=33, seed=5)
    b = KernelMachinePredictor.random(7, 3, n_sv=33, seed=5)
    c = KernelMachinePredictor.random(7, 3, n_sv=33, seed=6)
    assert np.array_equal(a.alpha, b.alpha)
    assert not np.array_equal(a.alpha, c.alpha)
    assert np.allclose(np.abs(a.alpha).sum(axis=1), 4.0)
    assert a.gamma == 1.0 / 7 and a.n_out == 3 and a.n_sv == 33


# ----------------------------------------------------------------------- #
# sklearn

@pytest.mark.parametrize(
    "kind", ["svc_rbf", "svc_poly", "nusvc", "svr", "nusvr", "kr2", "kr_poly"])
def test_from_sklearn_matches_estimator(kind):
    est, rows, pred = _case(kind)
    score = est.decision_function if hasattr(est, "decision_function") \
        else est.predict
    want = np.asarray(score(rows), dtype=np.float64).reshape(len(rows), -1)
    got = pred(rows)
    assert pred.activation == "none"
    assert got.shape == want.shape == (80, 2 if kind == "kr2" else 1)
    assert np.allclose(got, want, rtol=0.0, atol=1e-10), np.abs(got - want).max()


def test_from_sklearn_reads_fitted_gamma():
    est, _, pred = _case("svc_rbf")
    assert est.gamma == "scale" and pred.gamma == est._gamma
    est, _, pred = _case("kr2")
    assert est.gamma is None and pred.gamma == 1.0 / D


def test_from_sklearn_sparse_support_vectors_are_densified():
    pytest.importorskip("sklearn")
    import scipy.sparse as sp
    from sklearn.svm import SVR

    X, _, score = _data()
    est = SVR(kernel="rbf", gamma=0.3).fit(sp.csr_matrix(X), score)
    assert sp.issparse(est.support_vectors_)
    pred = KernelMachinePredictor.from_sklearn(est)
    assert isinstance(pred.support_vectors, np.ndarray)
    assert np.allclose(pred(X[:20])[:, 0], est.predict(X[:20]),
                       rtol=0.0, atol=1e-10)


def test_from_sklearn_proba_is_the_closed_form_platt_sigmoid():
    est, rows, _ = _case("svc_proba")
    pred = KernelMachinePredictor.from_sklearn(est, output="proba")
    assert pred.n_out == 2 and pred.activation == "softmax"
    f = est.decision_function(rows)
    p1 = 1.0 / (1.0 + np.exp(est.probA_[0] * f - est.probB_[0]))
    got = pred(rows)
    assert np.allclose(got[:, 1], p1, rtol=0.0, atol=1e-12)
    assert np.allclose(got.sum(axis=1), 1.0, rtol=0.0, atol=1e-12)
    # libsvm's iterative coupling stays close to the closed form
    assert np.abs(got - est.predict_proba(rows)).max() < 2e-2
    # the sigmoid crosses 0.5 at f = probB / probA, not at f = 0 where
    # predict flips: the argmax can only agree with predict outside that
    # interval, so the estimator is one whose crossing lies within 0.1
    assert abs(est.probB_[0] / est.probA_[0]) < 0.1
    sure = np.abs(f) > 0.1
    assert sure.sum() > 20
    assert np.array_equal(est.classes_[got.argmax(axis=1)][sure],
                          est.predict(rows)[sure])


def test_from_sklearn_refuses_with_reason():
    pytest.importorskip("sklearn")
    from sklearn.kernel_ridge import KernelRidge
    from sklearn.svm import SVC, LinearSVC

    X, y, score = _data()
    y3 = np.digitize(score, [-0.7, 0.7])
    with pytest.raises(TypeError, match="multi-class"):
        KernelMachinePredictor.from_sklearn(SVC(kernel="rbf").fit(X, y3))
    with pytest.raises(TypeError, match="LinearPredictor"):
        KernelMachinePredictor.from_sklearn(SVC(kernel="linear").fit(X, y))
    with pytest.raises(TypeError, match="sigmoid"):
        KernelMachinePredictor.from_sklearn(SVC(kernel="sigmoid").fit(X, y))
    with pytest.raises(TypeError, match="precomputed"):
        KernelMachinePredictor.from_sklearn(
            SVC(kernel="precomputed").fit(X @ X.T, y))
    with pytest.raises(TypeError, match="callable"):
        KernelMachinePredictor.from_sklearn(
            SVC(kernel=lambda a, b: a @ b.T).fit(X, y))
    with pytest.raises(TypeError, match="9 targets"):
        KernelMachinePredictor.from_sklearn(
            KernelRidge(kernel="rbf").fit(X, np.tile(score[:, None], (1, 9))))
    with pytest.raises(TypeError, match="not a supported kernel machine"):
        KernelMachinePredictor.from_sklearn(LinearSVC().fit(X, y))
    with pytest.raises(TypeError, match="not a sklearn estimator"):
        KernelMachinePredictor.from_sklearn(object())
    with pytest.raises(TypeError, match="probability=True"):
        KernelMachinePredictor.from_sklearn(_case("svc_rbf")[0], output="proba")
    with pytest.raises(ValueError, match="unknown output"):
        KernelMachinePredictor.from_sklearn(_case("svc_rbf")[0], output="margin")


def test_from_sklearn_detects_parameters_that_do_not_reproduce():
    est = _fit("svr")
    est.intercept_ = est.intercept_ + 1e-6     # no longer what predict uses
    with pytest.raises(TypeError, match="do not reproduce"):
        KernelMachinePredictor.from_sklearn(est)


# ----------------------------------------------------------------------- #
# constructor, pickle, module, registry, loader

def test_constructor_validation():
    sv, al, ic = np.zeros((4, 3)), np.ones((2, 4)), np.zeros(2)
    KernelMachinePredictor(sv, al, ic, gamma=0.5)
    bad = [
        dict(support_vectors=np.zeros(4)),
        dict(alpha=np.ones((2, 5))),
        dict(alpha=np.ones(4)),
        dict(intercept=np.zeros(3)),
        dict(kernel="sigmoid"),
        dict(activation="tanh"),
        dict(gamma=0.0),
        dict(gamma=-1.0),
        dict(gamma=np.inf),
        dict(coef0=np.nan),
        dict(kernel="poly", degree=0),
        dict(kernel="poly", degree=2.5),
        dict(support_vectors=np.full((4, 3), np.nan)),
        dict(alpha=np.full((2, 4), np.inf)),
    ]
    for kw in bad:
        args = dict(support_vectors=sv, alpha=al, intercept=ic, gamma=0.5)
        args.update(kw)
        with pytest.raises(ValueError):
            KernelMachinePredictor(**args)


def test_pickle_round_trip_after_torch_module():
    """Predictors reach the distributed explainer's workers by pickle, also
    after a module has been built on them."""
    pred = KernelMachinePredictor.random(9, 3, n_sv=21, seed=4)
    X = np.random.Generator(np.random.Philox(key=[101, 0])).normal(size=(10, 9))
    assert pred.torch_module() is pred.torch_module()
    clone = pickle.loads(pickle.dumps(pred))
    assert clone._module is None
    assert np.array_equal(clone(X), pred(X))
    # a built module pickles too (TorchPredictor around build_module())
    mod = pickle.loads(pickle.dumps(pred.build_module()))
    with torch.no_grad():
        assert torch.equal(mod(torch.from_numpy(X)),
                           pred.torch_module()(torch.from_numpy(X)))


@pytest.mark.parametrize("kernel", ["rbf", "poly"])
@pytest.mark.parametrize("act", ["none", "sigmoid", "softmax"])
def test_torch_module_matches_call(kernel, act):
    pred = KernelMachinePredictor.random(9, 3, n_sv=37, kernel=kernel, seed=6,
                                         activation=act, coef0=0.5)
    X = np.random.Generator(np.random.Philox(key=[101, 1])).normal(size=(50, 9))
    with torch.no_grad():
        got = pred.torch_module()(torch.from_numpy(X).float()).double().numpy()
        got64 = pred.build_module(torch.float64)(torch.from_numpy(X)).numpy()
    assert got.shape == (50, 3)
    assert np.allclose(got, pred(X), rtol=0.0, atol=1e-5)
    assert np.allclose(got64, pred(X), rtol=0.0, atol=1e-12)


def test_make_predictor_kinds_agree():
    fused = make_predictor("svm_fused", 9, 3, seed=4, n_sv=21, kernel="poly")
    module = make_predictor("svm", 9, 3, seed=4, n_sv=21, kernel="poly",
                            device="cpu")
    assert isinstance(fused, KernelMachinePredictor)
    assert fused.kernel == "poly" and fused.n_sv == 21 and fused.n_out == 3
    mod = module.torch_module()
    assert np.array_equal(mod.alpha_t.double().numpy(),
                          fused.alpha.T.astype(np.float32).astype(np.float64))
    assert np.array_equal(mod.svt.double().numpy(),
                          fused.support_vectors.T.astype(np.float32).astype(np.float64))
    X = np.random.Generator(np.random.Philox(key=[101, 2])).normal(size=(12, 9))
    assert np.allclose(module(X), fused(X), rtol=0.0, atol=1e-5)


def test_load_model_wraps_pickled_svr(tmp_path):
    from distributedkernelshap_amd.utils import load_model

    est, rows, _ = _case("svr")
    path = tmp_path / "predictor.pkl"
    with open(path, "wb") as f:
        pickle.dump(est, f)
    pred = load_model(str(path))
    assert isinstance(pred, KernelMachinePredictor)
    assert np.allclose(pred(rows)[:, 0], est.predict(rows), rtol=0.0, atol=1e-10)


def test_load_model_keeps_linear_svc_linear_and_passes_refusals(tmp_path):
    pytest.importorskip("sklearn")
    from sklearn.svm import SVC

    from distributedkernelshap_amd.models import LinearPredictor
    from distributedkernelshap_amd.utils import load_model

    X, y, score = _data()
    path = tmp_path / "lin.pkl"
    with open(path, "wb") as f:
        pickle.dump(SVC(kernel="linear").fit(X, y), f)
    assert isinstance(load_model(str(path)), LinearPredictor)
    path = tmp_path / "multi.pkl"
    with open(path, "wb") as f:
        pickle.dump(SVC(kernel="rbf").fit(X, np.digitize(score, [-0.7, 0.7])), f)
    with pytest.raises(TypeError, match="multi-class"):
        load_model(str(path))


# ----------------------------------------------------------------------- #
# the fused kernel's operand images

@pytest.mark.parametrize("kernel", ["rbf", "poly"])
def test_fold_identity_on_blended_rows(kernel):
    """base + mask·(xp − bgp) from km_pack equals the explicit pre-activation
    of the blended row, in fp64, with uneven groups and a group that does not
    vary (its columns follow the background)."""
    rng = np.random.Generator(np.random.Philox(key=[103, kernel == "poly"]))
    d, groups = 9, [[0], [1, 2], [3], [4, 5, 6], [7, 8]]
    varying = np.array([0, 1, 3, 4])              # group 2 does not vary
    col_group = np.empty(d, dtype=np.int64)
    for gi, g in enumerate(groups):
        col_group[g] = gi
    pred = KernelMachinePredictor.random(d, 2, n_sv=19, kernel=kernel, seed=8,
                                         coef0=0.5)
    pack = km_pack.pack_machine(pred.kernel_machine_params(), col_group,
                                len(groups), "cpu")
    assert pack["vpad"] == 32
    x = rng.normal(size=(3, d))
    bg = rng.normal(size=(4, d))
    masks = rng.uniform(size=(3, 11, len(varying))) < 0.5
    vidx = torch.from_numpy(varying)
    xparts = km_pack.group_parts(pack, torch.from_numpy(x))
    bgparts = km_pack.group_parts(pack, torch.from_numpy(bg))
    assert xparts.shape == (3, 19, 5) and xparts.dtype == torch.float64
    sel_x = xparts[:, :, vidx].numpy()            # (B, V, M)
    sel_bg = bgparts[:, :, vidx].numpy()          # (N, V, M)
    base = bgparts.sum(dim=2).numpy()             # (N, V)
    pre = base[None, None] + np.einsum(
        "bsk,bnvk->bsnv", masks.astype(np.float64),
        sel_x[:, None] - sel_bg[None])
    # explicit: blend, then distance / dot product per support vector
    colv = np.full(len(groups), -1)
    colv[varying] = np.arange(len(varying))
    on = np.where(colv[col_group] >= 0,
                  masks[:, :, np.maximum(colv[col_group], 0)], False)
    rows = np.where(on[:, :, None, :], x[:, None, None, :], bg[None, None])
    sv = pred.support_vectors
    if kernel == "rbf":
        want = ((rows[..., None, :] - sv) ** 2).sum(axis=-1)
    else:
        want = rows @ sv.T
    assert np.abs(pre - want).max() < 1e-12
    # and the kernel of the folded value is the oracle's kernel value
    kv = np.exp(-pred.gamma * pre) if kernel == "rbf" \
        else (pred.gamma * pre + pred.coef0) ** pred.degree
    assert np.abs(kv - pred.kernel_values(rows.reshape(-1, d)).reshape(kv.shape)
                  ).max() < 1e-12

    # f32 images: padded rows / columns are zero, bgpn is negated
    xp = km_pack.image(pack, xparts, vidx)
    bgpn = km_pack.image(pack, bgparts, vidx, negate=True)
    bimg = km_pack.base(pack, bgparts)
    assert xp.shape == (3, 32, 16) and bgpn.shape == (4, 32, 16)
    assert bimg.shape == (4, 32) and xp.dtype == torch.float32
    assert not xp[:, 19:].any() and not xp[:, :, 4:].any()
    assert not bgpn[:, 19:].any() and not bgpn[:, :, 4:].any()
    assert not bimg[:, 19:].any()
    assert np.array_equal(xp[:, :19, :4].numpy(), sel_x.astype(np.float32))
    assert np.array_equal(bgpn[:, :19, :4].numpy(), (-sel_bg).astype(np.float32))
    assert np.array_equal(bimg[:, :19].numpy(), base.astype(np.float32))
    assert pack["alpha"].shape == (16, 32) and pack["intercept"].shape == (16,)
    assert not pack["alpha"][2:].any() and not pack["alpha"][:, 19:].any()
    assert np.array_equal(pack["alpha"][:2, :19].numpy(),
                          pred.alpha.astype(np.float32))


def test_envelope_reason_names_the_cause():
    ok = KernelMachinePredictor.random(5, 8, n_sv=2048, kernel="poly", degree=8)
    assert km_pack.envelope_reason(ok.kernel_machine_params()) is None
    many = KernelMachinePredictor.random(5, 2, n_sv=2049)
    assert "2049 support vectors" in km_pack.envelope_reason(
        many.kernel_machine_params())
    wide = KernelMachinePredictor.random(5, 9, n_sv=8)
    assert "n_out 9" in km_pack.envelope_reason(wide.kernel_machine_params())
    steep = KernelMachinePredictor.random(5, 2, n_sv=8, kernel="poly", degree=9)
    assert "degree 9" in km_pack.envelope_reason(steep.kernel_machine_params())


def test_instances_per_launch_stays_within_the_budget():
    pred = KernelMachinePredictor.random(64, 2, n_sv=2048)
    pack = km_pack.pack_machine(pred.kernel_machine_params(), np.arange(64),
                                64, "cpu")
    step = km_pack.instances_per_launch(pack, 64, 64)
    assert 1 <= step < 256
    assert step * 4 * 2048 * 64 <= km_pack.WORKSPACE_BYTES


# ----------------------------------------------------------------------- #
# CPU engine end to end

def test_cpu_engine_explains_a_kernel_machine():
    from distributedkernelshap_amd.core.engine import KernelShapEngine
    from distributedkernelshap_amd.core.links import logit

    pred = KernelMachinePredictor.random(D, 2, n_sv=30, seed=9)
    rng = np.random.Generator(np.random.Philox(key=[107, 0]))
    bg, X = rng.normal(size=(12, D)), rng.normal(size=(3, D))
    eng = KernelShapEngine(pred, bg, link="logit", seed=0, device="cpu")
    sv = eng.shap_values(X)
    fx = logit(pred(X))
    for o in range(2):
        assert sv[o].shape == (3, D)
        total = sv[o].sum(axis=1) + eng.expected_value[o]
        assert np.abs(total - fx[:, o]).max() < 1e-8
