"""TreeEnsemblePredictor on the CPU: agreement with sklearn (including rows
that sit on or next to a threshold), the torch module, the packed tables of
the fused kernel walked in numpy, and the registry / loader wiring."""
import pickle

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from distributedkernelshap_amd.models import (  # noqa: E402
    TreeEnsemblePredictor,
    make_predictor,
)
from distributedkernelshap_amd.ops import tree_pack  # noqa: E402

D = 6


def _data(n_classes=2):
    rng = np.random.Generator(np.random.Philox(key=[53, n_classes]))
    X = rng.normal(size=(300, D))
    score = X[:, 0] + 0.5 * X[:, 1] * X[:, 2] - X[:, 3]
    if n_classes == 2:
        y = (score > 0).astype(int)
    else:
        y = np.digitize(score, [-0.7, 0.7])
    return X, y, score


def _fit(kind):
    # only the tests that wrap an estimator need sklearn; the rest of this
    # file runs without it
    pytest.importorskip("sklearn")
    from sklearn.ensemble import (GradientBoostingClassifier,
                                  GradientBoostingRegressor,
                                  RandomForestClassifier)
    from sklearn.tree import DecisionTreeRegressor

    if kind == "gbc2":
        X, y, _ = _data(2)
        return GradientBoostingClassifier(
            n_estimators=20, max_depth=3, random_state=0).fit(X, y), X
    if kind == "gbc3":
        X, y, _ = _data(3)
        return GradientBoostingClassifier(
            n_estimators=10, max_depth=3, random_state=0).fit(X, y), X
    if kind == "gbr":
        X, _, score = _data(2)
        return GradientBoostingRegressor(
            n_estimators=20, max_depth=3, random_state=0).fit(X, score), X
    if kind == "rfc":
        X, y, _ = _data(3)
        return RandomForestClassifier(
            n_estimators=8, max_leaf_nodes=20, random_state=0).fit(X, y), X
    X, _, score = _data(2)
    return DecisionTreeRegressor(max_depth=5, random_state=0).fit(X, score), X


def _root(est):
    """(feature, threshold) of the first tree's root split."""
    tree = est
    if hasattr(est, "estimators_"):
        tree = np.asarray(est.estimators_, dtype=object).reshape(-1)[0]
    return int(tree.tree_.feature[0]), float(tree.tree_.threshold[0])


def _rows(est, X):
    """50 rows: 47 data rows, two a hair on either side of a root threshold
    (one value after the float32 rounding, so they take the same branch,
    which a float64 comparison would not give), one exactly on it."""
    rows = X[:50].copy()
    f, thr = _root(est)
    assert thr != 0.0
    rows[47, f] = thr * (1 + 1e-12)
    rows[48, f] = thr * (1 - 1e-12)
    rows[49, f] = thr
    return rows


KINDS = ["gbc2", "gbc3", "gbr", "rfc", "dtr"]
_FITTED = {}


def _case(kind):
    if kind not in _FITTED:
        est, X = _fit(kind)
        _FITTED[kind] = (est, _rows(est, X), TreeEnsemblePredictor.from_sklearn(est))
    return _FITTED[kind]


def _sk_out(est, rows):
    if hasattr(est, "predict_proba"):
        return est.predict_proba(rows)
    return est.predict(rows)[:, None]


@pytest.mark.parametrize("kind", KINDS)
def test_from_sklearn_matches_estimator(kind):
    est, rows, pred = _case(kind)
    want = _sk_out(est, rows)
    got = pred(rows)
    assert got.shape == want.shape
    assert np.allclose(got, want, rtol=0.0, atol=1e-12), np.abs(got - want).max()


def test_float32_rule_differs_from_float64_comparison():
    # the edge row is only a guard if the two rules really disagree on it
    est, rows, _ = _case("gbc2")
    f, thr = _root(est)
    edge = rows[47:50, f]
    naive = edge <= thr
    rule = edge.astype(np.float32).astype(np.float64) <= thr
    assert naive[0] != naive[1]          # the two rows straddle the threshold
    assert rule[0] == rule[1] == rule[2]  # after rounding they are one value
    assert (naive != rule).any()


@pytest.mark.parametrize("kind", KINDS)
def test_torch_module_matches_call(kind):
    _, rows, pred = _case(kind)
    with torch.no_grad():
        got = pred.torch_module()(torch.from_numpy(rows).float()).double().numpy()
    assert np.allclose(got, pred(rows), rtol=0.0, atol=1e-6)
    with torch.no_grad():
        got64 = pred.build_module(torch.float64)(torch.from_numpy(rows)).numpy()
    assert np.allclose(got64, pred(rows), rtol=0.0, atol=1e-12)


def _walk_packed(pack, dx, dbg, nm):
    """Pure numpy walk over the packed tables: (B, S, N, n_out) raw scores.
    ``nm`` (B, S, T) uint64 node masks, ``dx`` (B, T), ``dbg`` (N, T)."""
    child = pack["child"].numpy()
    meta = pack["meta"].numpy()
    leaves = pack["leaves"].numpy().astype(np.float64)
    b, s, n_trees = nm.shape
    n = dbg.shape[0]
    raw = np.zeros((b, s, n, pack["n_out"]))
    dx = dx.numpy().view(np.uint64)
    dbg = dbg.numpy().view(np.uint64)
    for bi in range(b):
        for si in range(s):
            for ni in range(n):
                for t in range(n_trees):
                    g = dbg[ni, t]
                    c = int(g ^ ((dx[bi, t] ^ g) & nm[bi, si, t]))
                    coff, loff, col, _ = meta[t]
                    node = 0
                    while node < 64:
                        node = int(child[coff + node, (c >> node) & 1])
                    v = leaves[loff + node - 64]
                    if pack["leaf_mode"] == 0:
                        raw[bi, si, ni, col] += v
                    else:
                        raw[bi, si, ni] += v
    return raw


def _node_masks(pack, masks, vmap):
    """nm[b, s, t]: OR of the node masks of tree t's groups that are on."""
    off = pack["grp_off"].numpy()
    gid = pack["grp_id"].numpy()
    gmask = pack["grp_mask"].numpy().view(np.uint64)
    b, s, _ = masks.shape
    nm = np.zeros((b, s, pack["n_trees"]), dtype=np.uint64)
    for t in range(pack["n_trees"]):
        for e in range(off[t], off[t + 1]):
            vi = vmap[gid[e]]
            if vi >= 0:
                nm[:, :, t] |= np.where(masks[:, :, vi] != 0, gmask[e],
                                        np.uint64(0))
    return nm


@pytest.mark.parametrize("vector_leaves", [False, True])
def test_packed_bit_walk_reproduces_call_on_blended_rows(vector_leaves):
    rng = np.random.Generator(np.random.Philox(key=[59, int(vector_leaves)]))
    d, groups = 7, [[0], [1, 2], [3], [4, 5, 6]]
    col_group = np.empty(d, dtype=np.int64)
    for gi, g in enumerate(groups):
        col_group[g] = gi
    pred = TreeEnsemblePredictor.random(
        d, 3, trees=6, depth=3, seed=3, activation="none",
        vector_leaves=vector_leaves)
    x = rng.normal(size=(2, d))
    bg = rng.normal(size=(3, d))
    bg[:, 3] = x[0, 3]            # group 2 does not vary: table entry -1
    vmap = np.array([0, 1, -1, 2])
    masks = (rng.uniform(size=(2, 5, 3)) < 0.5).astype(np.uint8)
    pack = tree_pack.pack_trees(pred.tree_params(), col_group, "cpu")
    dx = tree_pack.decision_bits(pack, torch.from_numpy(x))
    dbg = tree_pack.decision_bits(pack, torch.from_numpy(bg))
    raw = _walk_packed(pack, dx, dbg, _node_masks(pack, masks, vmap))
    got = pred.base + pred.scale * raw
    # explicit blend; the non-varying group takes the background everywhere
    full = np.zeros((2, 5, d), dtype=bool)
    for j in range(d):
        vi = vmap[col_group[j]]
        if vi >= 0:
            full[:, :, j] = masks[:, :, vi] != 0
    rows = np.where(full[:, :, None, :], x[:, None, None, :], bg[None, None])
    want = pred(rows.reshape(-1, d)).reshape(2, 5, 3, 3)
    # fp32 leaf table against fp64 leaves: 6 leaves of magnitude ~1
    assert np.allclose(got, want, rtol=0.0, atol=1e-6)


def test_single_leaf_tree_packs_and_walks():
    stump = {"feature": [-2], "threshold": [-2.0], "left": [-1], "right": [-1],
             "value": [0.25]}
    split = {"feature": [1, -2, -2], "threshold": [0.0, -2.0, -2.0],
             "left": [1, -1, -1], "right": [2, -1, -1], "value": [0.0, 1.0, -1.0]}
    pred = TreeEnsemblePredictor([stump, split], 2, 1)
    x = np.array([[0.0, -1.0], [0.0, 1.0]])
    assert np.allclose(pred(x)[:, 0], [1.25, -0.75])
    pack = tree_pack.pack_trees(pred.tree_params(), np.arange(2), "cpu")
    dx = tree_pack.decision_bits(pack, torch.from_numpy(x))
    nm = np.zeros((2, 1, 2), dtype=np.uint64)
    raw = _walk_packed(pack, dx, dx, nm)
    assert np.allclose(raw[0, 0, :, 0], [1.25, -0.75])


def test_from_sklearn_refuses_with_reason():
    pytest.importorskip("sklearn")
    from sklearn.ensemble import (GradientBoostingClassifier,
                                  HistGradientBoostingClassifier,
                                  RandomForestClassifier)
    from sklearn.linear_model import LogisticRegression

    X, y, _ = _data(2)
    hist = HistGradientBoostingClassifier(max_iter=3).fit(X, y)
    with pytest.raises(TypeError, match="HistGradientBoosting"):
        TreeEnsemblePredictor.from_sklearn(hist)
    multi = RandomForestClassifier(n_estimators=2, random_state=0).fit(
        X, np.stack([y, 1 - y], axis=1))
    with pytest.raises(TypeError, match="multi-output"):
        TreeEnsemblePredictor.from_sklearn(multi)
    gb_init = GradientBoostingClassifier(
        n_estimators=3, init=LogisticRegression(), random_state=0).fit(X, y)
    with pytest.raises(TypeError, match="non-constant init"):
        TreeEnsemblePredictor.from_sklearn(gb_init)
    gb_exp = GradientBoostingClassifier(
        n_estimators=3, loss="exponential", random_state=0).fit(X, y)
    with pytest.raises(TypeError, match="exponential"):
        TreeEnsemblePredictor.from_sklearn(gb_exp)
    with pytest.raises(TypeError, match="LogisticRegression"):
        TreeEnsemblePredictor.from_sklearn(LogisticRegression().fit(X, y))


def test_constructor_validation():
    ok = {"feature": [0, -2, -2], "threshold": [0.0, 0.0, 0.0],
          "left": [1, -1, -1], "right": [2, -1, -1], "value": [0.0, 1.0, 2.0]}
    TreeEnsemblePredictor([ok], 2, 1)
    with pytest.raises(ValueError, match="activation"):
        TreeEnsemblePredictor([ok], 2, 1, activation="tanh")
    with pytest.raises(ValueError, match="at least one tree"):
        TreeEnsemblePredictor([], 2, 1)
    with pytest.raises(ValueError, match="equally long"):
        TreeEnsemblePredictor([dict(ok, threshold=[0.0])], 2, 1)
    with pytest.raises(ValueError, match="out of range"):
        TreeEnsemblePredictor([dict(ok, feature=[5, -2, -2])], 2, 1)
    with pytest.raises(ValueError, match="rooted at node 0"):
        TreeEnsemblePredictor([dict(ok, right=[1, -1, -1])], 2, 1)
    with pytest.raises(ValueError, match="out_col"):
        TreeEnsemblePredictor([ok], 2, 2, out_col=[2])
    with pytest.raises(ValueError, match="base"):
        TreeEnsemblePredictor([ok], 2, 2, base=[0.0])
    vec = dict(ok, value=np.zeros((3, 2)))
    with pytest.raises(ValueError, match="same leaf form"):
        TreeEnsemblePredictor([ok, vec], 2, 2)
    with pytest.raises(ValueError, match="vector leaves"):
        TreeEnsemblePredictor([vec], 2, 2, out_col=[0])


def test_load_model_wraps_pickled_gradient_boosting(tmp_path):
    from distributedkernelshap_amd.utils import load_model

    est, rows, _ = _case("gbc2")
    path = tmp_path / "predictor.pkl"
    with open(path, "wb") as f:
        pickle.dump(est, f)
    pred = load_model(str(path))
    assert isinstance(pred, TreeEnsemblePredictor)
    assert np.allclose(pred(rows), est.predict_proba(rows), rtol=0.0, atol=1e-12)


def test_pickle_round_trip_after_torch_module():
    """Predictors reach the distributed explainer's workers by pickle, also
    after a module has been built on them."""
    pred = TreeEnsemblePredictor.random(9, 3, trees=12, depth=3, seed=4)
    rng = np.random.Generator(np.random.Philox(key=[61, 1]))
    X = rng.normal(size=(40, 9))
    want = pred(X)
    pred.torch_module()
    clone = pickle.loads(pickle.dumps(pred))
    assert isinstance(clone, TreeEnsemblePredictor)
    assert clone._module is None and clone._flat is None   # caches dropped
    assert np.array_equal(clone(X), want)
    with torch.no_grad():
        got = clone.torch_module()(torch.from_numpy(X).float()).double().numpy()
    assert np.allclose(got, want, rtol=0.0, atol=1e-6)
    # the module itself, and the TorchPredictor around it
    mod = pickle.loads(pickle.dumps(pred.build_module(torch.float64)))
    with torch.no_grad():
        assert np.allclose(mod(torch.from_numpy(X)).numpy(), want,
                           rtol=0.0, atol=1e-12)
    wrapped = make_predictor("trees", 9, 3, seed=4, trees=12, depth=3,
                             device="cpu")
    wrapped(X)
    clone = pickle.loads(pickle.dumps(wrapped))
    assert np.array_equal(clone(X), wrapped(X))
    assert np.allclose(clone(X), want, rtol=0.0, atol=1e-6)


def test_nan_input_is_refused():
    pred = TreeEnsemblePredictor.random(5, 2, trees=3, depth=2)
    X = np.zeros((2, 5))
    X[1, 3] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        pred(X)


def test_make_predictor_kinds_agree():
    fused = make_predictor("trees_fused", 9, 3, seed=4, trees=12, depth=3)
    module = make_predictor("trees", 9, 3, seed=4, trees=12, depth=3,
                            device="cpu")
    assert isinstance(fused, TreeEnsemblePredictor)
    rng = np.random.Generator(np.random.Philox(key=[61, 0]))
    X = rng.normal(size=(40, 9))
    assert np.allclose(module(X), fused(X), rtol=0.0, atol=1e-6)
    # non-complete trees: some branch ends above the full depth
    sizes = [len(t["feature"]) for t in fused.trees]
    assert min(sizes) < 2 ** 4 - 1


def _chain(n_internal, d):
    """Degenerate chain: every internal node's right child is the next split,
    its left child a leaf (depth = n_internal)."""
    n_nodes = 2 * n_internal + 1
    feat = np.full(n_nodes, -2)
    thr = np.zeros(n_nodes)
    left = np.full(n_nodes, -1)
    right = np.full(n_nodes, -1)
    for i in range(n_internal):
        feat[2 * i] = i % d
        thr[2 * i] = -1.5 + 3.0 * i / n_internal
        left[2 * i] = 2 * i + 1
        right[2 * i] = 2 * i + 2
    return {"feature": feat, "threshold": thr, "left": left, "right": right,
            "value": np.linspace(-1.0, 1.0, n_nodes)}


def test_envelope_reason_names_the_cause():
    ok = TreeEnsemblePredictor([_chain(64, 5)], 5, 1)
    assert tree_pack.envelope_reason(ok.tree_params()) is None
    deep = TreeEnsemblePredictor([_chain(3, 5), _chain(65, 5)], 5, 1)
    reason = tree_pack.envelope_reason(deep.tree_params())
    assert "tree 1" in reason and "65 internal nodes" in reason
    wide = TreeEnsemblePredictor([_chain(2, 5)], 5, 9)
    assert "n_out 9" in tree_pack.envelope_reason(wide.tree_params())
    many = TreeEnsemblePredictor([_chain(1, 5)] * 1025, 5, 1)
    assert "1025 trees" in tree_pack.envelope_reason(many.tree_params())
