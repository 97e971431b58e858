"""MLPPredictor (CPU side): numpy fp64 forward vs torch, from_torch,
make_predictor("mlp_fused"), load_model on sklearn MLPClassifier, and the CPU
engine's local accuracy with an MLP."""
import pickle

import numpy as np
import pytest

torch = pytest.importorskip("torch")
nn = torch.nn

from distributedkernelshap_amd.models import MLPPredictor, make_predictor  # noqa: E402


def _sequential_f64(pred):
    """fp64 nn.Sequential built independently from the predictor's arrays."""
    weights, biases, hid, act = pred.mlp_params()
    mods = []
    for i, (w, b) in enumerate(zip(weights, biases)):
        lin = nn.Linear(w.shape[1], w.shape[0]).double()
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(w))
            lin.bias.copy_(torch.from_numpy(b))
        mods.append(lin)
        if i < len(weights) - 1:
            mods.append({"relu": nn.ReLU(), "tanh": nn.Tanh()}[hid])
    if act == "softmax":
        mods.append(nn.Softmax(dim=-1))
    elif act == "sigmoid":
        mods.append(nn.Sigmoid())
    return nn.Sequential(*mods)


@pytest.mark.parametrize("hidden_activation", ["relu", "tanh"])
@pytest.mark.parametrize("activation", ["softmax", "sigmoid", "none"])
@pytest.mark.parametrize("layers", [1, 2, 3])
def test_call_matches_fp64_torch(hidden_activation, activation, layers):
    pred = MLPPredictor.random(
        7, 3, hidden=12, layers=layers, seed=layers,
        activation=activation, hidden_activation=hidden_activation,
    )
    assert pred.n_out == 3
    rng = np.random.Generator(np.random.Philox(key=[1, layers]))
    X = rng.normal(size=(33, 7))
    with torch.no_grad():
        ref = _sequential_f64(pred)(torch.from_numpy(X)).numpy()
    out = pred(X)
    assert out.dtype == np.float64 and out.shape == (33, 3)
    assert np.allclose(out, ref, rtol=0.0, atol=1e-12)


def test_from_torch_round_trip():
    pred = MLPPredictor.random(5, 2, hidden=8, layers=2, seed=4,
                               activation="sigmoid", hidden_activation="tanh")
    back = MLPPredictor.from_torch(_sequential_f64(pred))
    assert back.activation == "sigmoid" and back.hidden_activation == "tanh"
    assert len(back.weights) == 3
    for a, b in zip(pred.weights + pred.biases, back.weights + back.biases):
        assert np.array_equal(a, b)
    # and through the predictor's own cached fp32 module
    mod = pred.torch_module()
    assert mod is pred.torch_module()
    again = MLPPredictor.from_torch(mod)
    for a, b in zip(pred.weights, again.weights):
        assert np.allclose(a, b, rtol=0.0, atol=1e-6)


def test_from_torch_rejects_other_modules():
    bad = nn.Sequential(nn.Conv1d(1, 1, 3), nn.ReLU(), nn.Linear(4, 2))
    with pytest.raises(TypeError):
        MLPPredictor.from_torch(bad)
    with pytest.raises(TypeError):
        MLPPredictor.from_torch(
            nn.Sequential(nn.Linear(4, 4), nn.ReLU(), nn.Conv1d(1, 1, 3))
        )


def test_make_predictor_mlp_fused_matches_mlp():
    fused = make_predictor("mlp_fused", 8, 2, seed=3, hidden=16, layers=2)
    module = make_predictor("mlp", 8, 2, seed=3, hidden=16, layers=2, device="cpu")
    assert isinstance(fused, MLPPredictor)
    assert [w.shape for w in fused.weights] == [(16, 8), (16, 16), (2, 16)]
    rng = np.random.Generator(np.random.Philox(key=[3, 3]))
    X = rng.normal(size=(50, 8))
    assert np.allclose(fused(X), module(X), rtol=0.0, atol=1e-5)


def test_make_predictor_unknown_kind_still_raises():
    with pytest.raises(ValueError):
        make_predictor("mlp_fusedd", 4)


@pytest.mark.parametrize("n_classes", [2, 3])
def test_load_model_wraps_sklearn_mlp(tmp_path, n_classes):
    sk = pytest.importorskip("sklearn.neural_network")
    import warnings

    from distributedkernelshap_amd.utils import load_model

    rng = np.random.Generator(np.random.Philox(key=[6, n_classes]))
    X = rng.normal(size=(60, 5))
    y = np.arange(60) % n_classes
    clf = sk.MLPClassifier(hidden_layer_sizes=(8,), max_iter=50, random_state=0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # 50 iterations: ConvergenceWarning
        clf.fit(X, y)
    path = tmp_path / "predictor.pkl"
    with open(path, "wb") as f:
        pickle.dump(clf, f)
    pred = load_model(str(path))
    assert isinstance(pred, MLPPredictor)
    assert pred.n_out == n_classes
    assert pred.activation == "softmax" and pred.hidden_activation == "relu"
    assert np.allclose(pred(X), clf.predict_proba(X), rtol=0.0, atol=1e-10)


def test_cpu_engine_local_accuracy():
    from distributedkernelshap_amd.core.engine import KernelShapEngine
    from distributedkernelshap_amd.core.links import logit

    d = 6
    pred = MLPPredictor.random(d, 2, hidden=16, layers=2, seed=2)
    rng = np.random.Generator(np.random.Philox(key=[2, 6]))
    bg = rng.normal(size=(20, d))
    X = rng.normal(size=(3, d))
    eng = KernelShapEngine(pred, bg, link="logit", seed=0, device="cpu")
    sv = eng.shap_values(X)  # 2^6 - 2 coalitions: full enumeration
    fx = logit(pred(X))
    for o in range(2):
        total = sv[o].sum(axis=1) + eng.expected_value[o]
        assert np.abs(total - fx[:, o]).max() < 1e-9
