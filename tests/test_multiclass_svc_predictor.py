"""MulticlassSVCPredictor on the CPU: the fp64 oracle against sklearn's public
API, the torch module against the oracle (including on the inputs of the GPU
kernel tests: the yardstick for their bounds), the fused kernel's envelope,
and the CPU engine end to end."""
import pickle

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytest.importorskip("sklearn")

from multiclass_svc_cases import (  # noqa: E402
    ATOL, RTOL, SHAPES, case, module_fp32,
)

from distributedkernelshap_amd.models import (  # noqa: E402
    KernelMachinePredictor,
    MulticlassSVCPredictor,
    TorchPredictor,
    make_predictor,
)
from distributedkernelshap_amd.ops import km_pack  # noqa: E402

LABELS = np.array([2, 5, 9, 11, 12, 20])         # non-contiguous class labels


def _data(k):
    rng = np.random.Generator(np.random.Philox(key=[137, k]))
    X = rng.normal(size=(60 * k, 5))
    centres = 1.5 * rng.normal(size=(k, 5))
    cls = rng.integers(k, size=X.shape[0])
    return X + centres[cls], LABELS[cls], rng.normal(size=(40, 5)) * 1.5


_FITS = {}


def _fit(name, k, kernel, shape="ovr"):
    """Fitted estimator (probability=True) and probe rows, fitted once."""
    key = (name, k, kernel, shape)
    if key not in _FITS:
        from sklearn.svm import SVC, NuSVC

        X, y, rows = _data(k)
        if name == "SVC":
            est = SVC(kernel=kernel, gamma=0.2, coef0=0.5, probability=True,
                      decision_function_shape=shape, random_state=0)
        else:
            est = NuSVC(nu=0.2, kernel=kernel, gamma=0.2, coef0=0.5,
                        probability=True, decision_function_shape=shape,
                        random_state=0)
        _FITS[key] = (est.fit(X, y), rows)
    return _FITS[key]


def _decision(est, rows, shape):
    old = est.decision_function_shape
    try:
        est.decision_function_shape = shape
        return est.decision_function(rows)
    finally:
        est.decision_function_shape = old


# ----------------------------------------------------------------------- #
# from_sklearn

@pytest.mark.parametrize("kernel", ["rbf", "poly"])
@pytest.mark.parametrize("k", [3, 4, 6])
@pytest.mark.parametrize("name", ["SVC", "NuSVC"])
def test_from_sklearn_reproduces_decision_function(name, k, kernel):
    est, rows = _fit(name, k, kernel)
    assert list(est.classes_) == list(LABELS[:k])
    for shape, width in (("ovo", k * (k - 1) // 2), ("ovr", k)):
        pred = MulticlassSVCPredictor.from_sklearn(est, output=shape)
        want = _decision(est, rows, shape)
        got = pred(rows)
        assert got.shape == want.shape == (40, width)
        assert pred.n_out == width and pred.n_raw == k * (k - 1) // 2
        assert np.abs(got - want).max() <= 1e-9 * (1.0 + np.abs(want).max())
    # raw() stays the pair decisions whatever the activation
    assert np.array_equal(pred.raw(rows), MulticlassSVCPredictor.from_sklearn(
        est, output="ovo")(rows))


def test_from_sklearn_decision_follows_the_estimators_shape():
    for shape, act, width in (("ovo", "none", 6), ("ovr", "ovr", 4)):
        est, rows = _fit("SVC", 4, "rbf", shape)
        pred = MulticlassSVCPredictor.from_sklearn(est)
        assert pred.activation == act and pred.n_out == width
        want = est.decision_function(rows)
        assert np.abs(pred(rows) - want).max() <= 1e-9 * (1 + np.abs(want).max())


def test_outputs_follow_classes_order_with_noncontiguous_labels():
    est, rows = _fit("SVC", 3, "rbf")
    assert list(est.classes_) == [2, 5, 9]
    pred = MulticlassSVCPredictor.from_sklearn(est, output="ovr")
    assert np.array_equal(est.classes_[pred(rows).argmax(axis=1)],
                          est.predict(rows))


@pytest.mark.parametrize("kernel", ["rbf", "poly"])
@pytest.mark.parametrize("k", [3, 4, 6])
def test_from_sklearn_proba(k, kernel):
    """libsvm stops its coupling iteration at eps = 0.005/K; the oracle is
    the fixed point. Measured gap: 3.0e-3."""
    est, rows = _fit("SVC", k, kernel)
    pred = MulticlassSVCPredictor.from_sklearn(est, output="proba")
    assert pred.activation == "coupling" and pred.n_out == k
    got = pred(rows)
    lib = est.predict_proba(rows)
    assert np.abs(got.sum(axis=1) - 1.0).max() < 1e-12
    assert (got > 0.0).all() and (got < 1.0).all()
    gap = np.abs(got - lib).max()
    print(f"K={k} {kernel}: max |oracle - predict_proba| = {gap:.2e}")
    assert gap < 1e-2
    top = np.sort(lib, axis=1)
    clear = top[:, -1] - top[:, -2] > 2e-2
    assert clear.any()
    assert np.array_equal(got.argmax(axis=1)[clear], lib.argmax(axis=1)[clear])


def test_from_sklearn_sparse_fit():
    import scipy.sparse as sp
    from sklearn.svm import SVC

    X, y, rows = _data(3)
    est = SVC(kernel="rbf", gamma=0.2).fit(sp.csr_matrix(X), y)
    assert sp.issparse(est.support_vectors_)
    pred = MulticlassSVCPredictor.from_sklearn(est, output="ovr")
    want = est.decision_function(rows)
    assert np.abs(pred(rows) - want).max() <= 1e-9 * (1 + np.abs(want).max())


def test_from_sklearn_refusals_name_the_reason():
    from sklearn.svm import SVC, SVR

    X, y, _ = _data(3)
    binary = SVC(kernel="rbf").fit(X, y == y[0])
    with pytest.raises(TypeError, match="KernelMachinePredictor"):
        MulticlassSVCPredictor.from_sklearn(binary)
    with pytest.raises(TypeError, match="probability=True"):
        MulticlassSVCPredictor.from_sklearn(
            SVC(kernel="rbf").fit(X, y), output="proba")
    with pytest.raises(TypeError, match="linear"):
        MulticlassSVCPredictor.from_sklearn(SVC(kernel="linear").fit(X, y))
    with pytest.raises(TypeError, match="sigmoid"):
        MulticlassSVCPredictor.from_sklearn(SVC(kernel="sigmoid").fit(X, y))
    with pytest.raises(TypeError, match="callable"):
        MulticlassSVCPredictor.from_sklearn(
            SVC(kernel=lambda a, b: a @ b.T).fit(X, y))
    with pytest.raises(TypeError, match="precomputed"):
        MulticlassSVCPredictor.from_sklearn(
            SVC(kernel="precomputed").fit(X @ X.T, y))
    with pytest.raises(TypeError, match="SVR"):
        MulticlassSVCPredictor.from_sklearn(SVR().fit(X, y))
    with pytest.raises(TypeError, match="not a sklearn"):
        MulticlassSVCPredictor.from_sklearn(object())
    with pytest.raises(ValueError, match="margin"):
        MulticlassSVCPredictor.from_sklearn(SVC().fit(X, y), output="margin")
    # the base class keeps refusing, and now points here
    with pytest.raises(TypeError, match="multi-class.*MulticlassSVCPredictor"):
        KernelMachinePredictor.from_sklearn(SVC(kernel="rbf").fit(X, y))


def test_constructor_validation():
    good = MulticlassSVCPredictor.random(5, 3, n_sv=12, activation="coupling")
    args = (good.support_vectors, good.alpha, good.intercept)
    with pytest.raises(ValueError, match="n_classes"):
        MulticlassSVCPredictor(*args, 2)
    with pytest.raises(ValueError, match="P = K"):
        MulticlassSVCPredictor(*args, 4)
    with pytest.raises(ValueError, match="activation"):
        MulticlassSVCPredictor(*args, 3, activation="softmax")
    with pytest.raises(ValueError, match="prob_a"):
        MulticlassSVCPredictor(*args, 3, activation="coupling")
    with pytest.raises(ValueError, match="P entries"):
        MulticlassSVCPredictor(*args, 3, activation="coupling",
                               prob_a=[-1.0], prob_b=[0.0])


# ----------------------------------------------------------------------- #
# random machines, the torch module

def test_random_has_the_libsvm_structure():
    a = MulticlassSVCPredictor.random(7, 4, n_sv=33, seed=5)
    b = MulticlassSVCPredictor.random(7, 4, n_sv=33, seed=5)
    c = MulticlassSVCPredictor.random(7, 4, n_sv=33, seed=6)
    assert np.array_equal(a.alpha, b.alpha) and not np.array_equal(a.alpha, c.alpha)
    assert a.alpha.shape == (6, 33) and a.n_raw == 6 and a.n_out == 4
    assert np.allclose(np.abs(a.alpha).sum(axis=1), 4.0)
    cuts = np.linspace(0, 33, 5).round().astype(int)
    for p, (i, j) in enumerate(zip(*np.triu_indices(4, 1))):
        on = np.zeros(33, dtype=bool)
        on[cuts[i] : cuts[i + 1]] = on[cuts[j] : cuts[j + 1]] = True
        assert (a.alpha[p][on] != 0).all() and not a.alpha[p][~on].any()
    coup = MulticlassSVCPredictor.random(7, 4, n_sv=33, seed=5,
                                         activation="coupling")
    assert (coup.prob_a < 0).all() and np.abs(coup.prob_b).max() <= 0.1
    assert MulticlassSVCPredictor.random(7, 4, n_sv=33, seed=5,
                                         activation="none").n_out == 6


def test_oracle_ovr_ties_go_to_the_first_class():
    pred = MulticlassSVCPredictor.random(5, 3, n_sv=12)
    out = pred.ovr(np.zeros((1, 3)))
    assert np.array_equal(out, [[2.0, 1.0, 0.0]])


@pytest.mark.parametrize("kernel", ["rbf", "poly"])
@pytest.mark.parametrize("act", ["none", "ovr", "coupling"])
@pytest.mark.parametrize("k", [3, 4, 6])
def test_torch_module_matches_oracle(k, act, kernel):
    pred = MulticlassSVCPredictor.random(9, k, n_sv=37, kernel=kernel, seed=6,
                                         activation=act, coef0=0.5)
    X = np.random.Generator(np.random.Philox(key=[139, k])).normal(size=(400, 9))
    ref = pred(X)
    with torch.no_grad():
        got = pred.torch_module()(torch.from_numpy(X).float()).double().numpy()
        got64 = pred.build_module(torch.float64)(torch.from_numpy(X)).numpy()
    assert got.shape == ref.shape == (400, pred.n_out)
    keep = np.ones(400, dtype=bool)
    if act == "ovr":
        keep = (np.abs(pred.raw(X)) >= 1e-4).all(axis=1)
        assert keep.mean() > 0.9
    err = np.abs(got - ref)[keep].max()
    print(f"K={k} {act} {kernel}: fp32 module max abs err = {err:.2e}")
    assert err < 1e-5
    assert np.abs(got64 - ref).max() < 1e-10


@pytest.mark.parametrize("shape_id", sorted(SHAPES))
def test_fp32_module_is_within_a_quarter_of_the_fused_bound(shape_id):
    """The yardstick of ``test_gpu_kernel_machine_multiclass.py``: on the very
    inputs of the kernel tests the fp32 module is within a quarter of the
    project's fused-predict bound, so that bound applies to the kernel.
    Measured: shape 6 (clip-saturated coupling) 8.4e-7, 1.6 % of the bound;
    every other shape below 2.4e-7 and 0.2 % of it."""
    p, ref, keep = case(shape_id)
    assert keep.mean() >= 0.9
    err = np.abs(module_fp32(p) - ref)
    ratio = (err / (ATOL + RTOL * np.abs(ref)))[keep].max()
    print(f"shape {shape_id}: fp32 module max abs err {err[keep].max():.2e}, "
          f"{ratio:.2%} of the bound, left out {1 - keep.mean():.2%}")
    assert ratio <= 0.25


def test_coupling_algorithm_in_fp32_on_saturating_pair_decisions():
    """The module's partially pivoted LU in fp32 against the fp64 minimiser,
    pair decisions drawn directly at scales 1, 4 and 12 (the last saturates
    the clip). Probabilities are at most 1 and fp32 eps is 6e-8; a pivoted
    7 x 7 solve behind an fp32 sigmoid should stay within a few eps, and the
    bound, 1e-6 = 16 eps, is a twentieth of the fused bound's atol.
    Measured: at most 2.0e-7 (libsvm's own sweep, 25 fixed sweeps in fp32
    numpy on the same inputs: 2.1e-6)."""
    worst = 0.0
    for k in (3, 4, 6):
        pred = MulticlassSVCPredictor.random(5, k, n_sv=12, seed=k,
                                             activation="coupling")
        mod = pred.build_module()
        rng = np.random.Generator(np.random.Philox(key=[149, k]))
        for scale in (1.0, 4.0, 12.0):
            f = scale * rng.normal(size=(300, pred.n_raw))
            with torch.no_grad():
                got = mod._coupling(torch.from_numpy(f).float()).double().numpy()
            ref = pred.coupling(f.astype(np.float32).astype(np.float64))
            worst = max(worst, np.abs(got - ref).max())
    print(f"fp32 LU coupling: max abs err vs fp64 minimiser = {worst:.2e}")
    assert worst < 1e-6


def test_pickle_round_trip_drops_the_module_cache():
    pred = MulticlassSVCPredictor.random(9, 4, n_sv=21, seed=4,
                                         activation="coupling")
    X = np.random.Generator(np.random.Philox(key=[139, 0])).normal(size=(6, 9))
    pred.torch_module()
    assert pred._module is not None
    clone = pickle.loads(pickle.dumps(pred))
    assert clone._module is None and clone.n_classes == 4
    assert np.array_equal(clone(X), pred(X))
    mod = pickle.loads(pickle.dumps(pred.build_module()))
    with torch.no_grad():
        assert torch.equal(mod(torch.from_numpy(X).float()),
                           pred.torch_module()(torch.from_numpy(X).float()))


def test_make_predictor_kinds_agree():
    fused = make_predictor("svm_multiclass_fused", 9, 4, seed=4, n_sv=21)
    module = make_predictor("svm_multiclass", 9, 4, seed=4, n_sv=21,
                            device="cpu")
    assert isinstance(fused, MulticlassSVCPredictor)
    assert isinstance(module, TorchPredictor)
    assert fused.n_classes == 4 and fused.activation == "coupling"
    X = np.random.Generator(np.random.Philox(key=[139, 2])).normal(size=(12, 9))
    assert np.allclose(module(X), fused(X), rtol=0.0, atol=1e-5)
    plain = make_predictor("svm_multiclass_fused", 9, 4, seed=4, n_sv=21,
                           activation="none")
    assert plain.n_out == 6 and np.array_equal(plain.alpha, fused.alpha)


# ----------------------------------------------------------------------- #
# the fused kernel's envelope and pack

def test_envelope_reason_for_pair_activations():
    def reason(k, act):
        pred = MulticlassSVCPredictor.random(5, k, n_sv=24, activation=act)
        return km_pack.envelope_reason(pred.kernel_machine_params())

    assert reason(6, "coupling") is None
    assert reason(6, "ovr") is None
    assert "7 classes (supported: <= 6)" in reason(7, "coupling")
    assert "7 classes" in reason(7, "ovr")
    assert "n_out 10" in reason(5, "none")            # P = 10 > 8
    assert reason(4, "none") is None                  # P = 6


def test_pack_carries_the_pair_operands():
    pred = MulticlassSVCPredictor.random(5, 4, n_sv=24, activation="coupling")
    params = pred.kernel_machine_params()
    assert params["n_classes"] == 4
    pack = km_pack.pack_machine(params, np.arange(5), 5, "cpu")
    assert pack["n_classes"] == 4 and pack["n_out"] == 6
    assert pack["prob_a"].shape == (16,) and pack["prob_a"].dtype == torch.float32
    assert np.array_equal(pack["prob_a"][:6].numpy(),
                          pred.prob_a.astype(np.float32))
    assert np.array_equal(pack["prob_b"][:6].numpy(),
                          pred.prob_b.astype(np.float32))
    assert not pack["prob_a"][6:].any() and not pack["alpha"][6:].any()
    assert km_pack.ACT_CODE["ovr"] == 3 and km_pack.ACT_CODE["coupling"] == 4


# ----------------------------------------------------------------------- #
# CPU engine end to end

def test_cpu_engine_explains_a_multiclass_svc():
    from distributedkernelshap_amd.core.engine import KernelShapEngine
    from distributedkernelshap_amd.core.links import logit

    d = 8
    pred = MulticlassSVCPredictor.random(d, 3, n_sv=30, seed=9,
                                         activation="coupling")
    rng = np.random.Generator(np.random.Philox(key=[139, 3]))
    bg, X = rng.normal(size=(12, d)), rng.normal(size=(3, d))
    eng = KernelShapEngine(pred, bg, link="logit", seed=0, device="cpu")
    sv = eng.shap_values(X)
    fx = logit(pred(X))
    assert len(sv) == 3
    for o in range(3):
        assert sv[o].shape == (3, d)
        total = sv[o].sum(axis=1) + eng.expected_value[o]
        assert np.abs(total - fx[:, o]).max() < 1e-8
