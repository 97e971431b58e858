"""RoutedTreeEnsemblePredictor on the CPU: agreement with sklearn
(HistGradientBoosting with native categorical columns, a forest fitted on
data with NaN), the routing rule on hand-built trees, the torch modules, the
packed tables of both fused kernels decoded in numpy, and the loader."""
import pickle

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from distributedkernelshap_amd.models import (  # noqa: E402
    RoutedTreeEnsemblePredictor,
    TreeEnsemblePredictor,
)
from distributedkernelshap_amd.ops import tree_pack  # noqa: E402

NAN = float("nan")
D = 6
CAT_A = np.arange(6.0)                            # feature 4
CAT_B = np.array([3.0, 7.0, 10.0, 20.0, 41.0])    # feature 5: not contiguous


# ----------------------------------------------------------------------- #
# against sklearn

def _data(n_classes=2, n=500):
    """float32-representable rows: four numeric columns (0 and 1 with NaN,
    2 and 3 never missing) and two categorical ones (4 with NaN)."""
    rng = np.random.Generator(np.random.Philox(key=[59, n_classes]))
    X = rng.normal(size=(n, D)).astype(np.float32).astype(np.float64)
    X[:, 4] = rng.choice(CAT_A, size=n)
    X[:, 5] = rng.choice(CAT_B, size=n)
    score = (X[:, 0] + 0.5 * X[:, 1] * X[:, 2] - X[:, 3]
             + 1.5 * np.isin(X[:, 4], [1.0, 4.0]) - 1.2 * np.isin(X[:, 5], [7.0, 41.0]))
    for col, share in ((0, 0.15), (1, 0.1), (4, 0.1)):
        gone = rng.uniform(size=n) < share
        X[gone, col] = NAN
        score[gone] += 0.8          # missingness carries signal
    y = (score > 0.3).astype(int) if n_classes == 2 \
        else np.digitize(score, [-0.6, 1.0])
    return X, y, score


def _fit(kind):
    pytest.importorskip("sklearn")
    from sklearn.ensemble import (HistGradientBoostingClassifier,
                                  HistGradientBoostingRegressor,
                                  RandomForestClassifier)

    if kind == "hgbc2":
        X, y, _ = _data(2)
        return HistGradientBoostingClassifier(
            max_iter=20, categorical_features=[4, 5], random_state=0).fit(X, y), X
    if kind == "hgbc3":
        X, y, _ = _data(3)
        return HistGradientBoostingClassifier(
            max_iter=8, categorical_features=[4, 5], random_state=0).fit(X, y), X
    if kind == "hgbr":
        X, _, score = _data(2)
        return HistGradientBoostingRegressor(
            max_iter=20, categorical_features=[4, 5], random_state=0).fit(X, score), X
    X, y, _ = _data(3)
    return RandomForestClassifier(
        n_estimators=8, max_leaf_nodes=24, random_state=0).fit(X, y), X


def _rows(X):
    """60 training rows (NaN in columns 0, 1 and 4 among them) and edge
    rows: NaN in every column in turn (2, 3 and 5 were never missing in
    training), an unknown, a negative, a fractional and a >= 256 category."""
    rows = [X[:60]]
    base = X[60:80].copy()
    base[np.isnan(base)] = 0.0
    for col in range(D):
        r = base[:3].copy()
        r[:, col] = NAN
        rows.append(r)
    for col, val in ((5, 5.0), (5, 42.0), (4, -1.0), (5, -3.0), (4, 300.0),
                     (5, 256.0), (4, 2.5), (4, 1e9), (5, 1e30)):
        r = base[3:6].copy()
        r[:, col] = val
        rows.append(r)
    allnan = np.full((1, D), NAN)
    return np.concatenate(rows + [allnan])


KINDS = ["hgbc2", "hgbc3", "hgbr", "rfc"]
_FITTED = {}


def _case(kind):
    if kind not in _FITTED:
        est, X = _fit(kind)
        _FITTED[kind] = (est, _rows(X),
                         RoutedTreeEnsemblePredictor.from_sklearn(est))
    return _FITTED[kind]


def _sk_out(est, rows):
    if hasattr(est, "predict_proba"):
        return est.predict_proba(rows)
    return est.predict(rows)[:, None]


@pytest.mark.parametrize("kind", KINDS)
def test_from_sklearn_matches_estimator(kind):
    est, rows, pred = _case(kind)
    assert isinstance(pred, TreeEnsemblePredictor)
    assert np.isnan(rows).any(axis=0).all()
    want = _sk_out(est, rows)
    got = pred(rows)
    assert got.shape == want.shape
    assert np.allclose(got, want, rtol=0.0, atol=1e-12), np.abs(got - want).max()


@pytest.mark.parametrize("kind", KINDS)
def test_fitted_models_use_the_routing(kind):
    """The comparison above is vacuous on a model without routed nodes."""
    _, rows, pred = _case(kind)
    n_cat = sum(int((tr["cat_row"] >= 0).sum()) for tr in pred.trees)
    n_ml = sum(int(tr["missing_left"].sum()) for tr in pred.trees)
    n_mr = sum(int(((tr["left"] >= 0) & ~tr["missing_left"]).sum())
               for tr in pred.trees)
    assert n_ml >= 1 and n_mr >= 1
    if kind != "rfc":
        assert n_cat >= 1 and pred.cat_left.shape == (n_cat, 8)
        assert sorted(pred.categories) == [4, 5]
        assert np.array_equal(pred.categories[4], CAT_A)       # NaN dropped
        assert np.array_equal(pred.categories[5], CAT_B)
    # flipping every missing_left changes the answer on these rows
    flipped = _rebuild(pred, trees=[dict(tr, missing_left=~tr["missing_left"])
                                    for tr in pred.trees])
    assert np.abs(flipped(rows) - pred(rows)).max() > 1e-3


def _rebuild(pred, **kw):
    args = dict(trees=pred.trees, n_features=pred.n_features, n_out=pred.n_out,
                base=pred.base, scale=pred.scale, out_col=pred.out_col,
                activation=pred.activation, cat_left=pred.cat_left,
                categories=pred.categories)
    args.update(kw)
    return RoutedTreeEnsemblePredictor(**args)


def test_hgb_plus_inf_threshold_is_imported():
    """HGB writes 'non-missing left, missing right' as a +inf threshold; the
    regressor's trees on this data hold some, or the hand-built test below is
    the only guard."""
    found = 0
    for kind in ("hgbc2", "hgbc3", "hgbr"):
        pred = _case(kind)[2]
        found += sum(int(np.isinf(tr["threshold"]).sum()) for tr in pred.trees)
        assert all(np.all(tr["threshold"][tr["left"] >= 0] > -np.inf)
                   for tr in pred.trees)
    print("+inf thresholds in the fitted HGB models:", found)


def test_encode_replaces_known_categories():
    pred = _case("hgbc2")[2]
    X = np.zeros((6, D))
    X[:, 5] = [3.0, 41.0, 5.0, NAN, -3.0, 10.0]
    X[:, 0] = [0.1, NAN, 1e-9, 0.0, 0.0, 0.0]
    enc = pred.encode(X)
    assert np.array_equal(enc[:, 5], [0.0, 4.0, NAN, NAN, NAN, 2.0], equal_nan=True)
    assert np.array_equal(enc[:, 4], np.zeros(6))              # 0.0 is code 0
    assert enc[0, 0] == float(np.float32(0.1)) and np.isnan(enc[1, 0])


# ----------------------------------------------------------------------- #
# the routing rule on hand-built trees

def _stump(feature, thr, lo, hi, missing_left=False, cat_row=-1):
    return {"feature": [feature, -2, -2], "threshold": [thr, 0.0, 0.0],
            "left": [1, -1, -1], "right": [2, -1, -1], "value": [0.0, lo, hi],
            "missing_left": [missing_left, False, False],
            "cat_row": [cat_row, -1, -1]}


def _bitset(codes):
    row = np.zeros(8, dtype=np.uint32)
    for c in codes:
        row[c >> 5] |= np.uint32(1) << np.uint32(c & 31)
    return row


@pytest.mark.parametrize("missing_left", [False, True])
def test_plus_inf_threshold_routes_nan_both_ways(missing_left):
    pred = RoutedTreeEnsemblePredictor(
        [_stump(0, np.inf, 1.0, 2.0, missing_left)], 1, 1)
    X = np.array([[NAN], [0.0], [-1e30], [3e38], [np.inf]])
    want = [1.0 if missing_left else 2.0, 1.0, 1.0, 1.0, 1.0]
    assert np.array_equal(pred.raw(X)[:, 0], want)


@pytest.mark.parametrize("missing_left", [False, True])
def test_categorical_node_word_boundaries(missing_left):
    left = [0, 3, 31, 32, 255]
    pred = RoutedTreeEnsemblePredictor(
        [_stump(0, 0.0, 1.0, 2.0, missing_left, cat_row=1)], 1, 1,
        cat_left=np.stack([_bitset(range(256)), _bitset(left)]))
    miss = 1.0 if missing_left else 2.0
    cases = {0.0: 1.0, 31.0: 1.0, 32.0: 1.0, 255.0: 1.0, 3.0: 1.0,
             1.0: 2.0, 30.0: 2.0, 33.0: 2.0, 63.0: 2.0, 64.0: 2.0, 254.0: 2.0,
             3.7: 1.0, 4.2: 2.0, 255.9: 1.0, 0.5: 1.0,       # truncation
             256.0: miss, -1.0: miss, -0.5: miss, 1e9: miss, np.inf: miss,
             -np.inf: miss, NAN: miss}
    X = np.array(list(cases))[:, None]
    assert np.array_equal(pred.raw(X)[:, 0], list(cases.values()))


def test_numeric_nan_does_not_take_the_compare():
    # a NaN compare is false: without the explicit test NaN would always go
    # right, whatever missing_left says
    pred = RoutedTreeEnsemblePredictor(
        [_stump(0, 0.5, 1.0, 2.0, True), _stump(1, 0.5, 10.0, 20.0, False)], 2, 1)
    X = np.array([[NAN, NAN], [0.0, 1.0], [1.0, 0.0]])
    assert np.array_equal(pred.raw(X)[:, 0], [21.0, 21.0, 12.0])


def test_without_routing_it_is_the_parent():
    plain = TreeEnsemblePredictor.random(9, 3, trees=12, depth=4, seed=4)
    routed = RoutedTreeEnsemblePredictor(
        plain.trees, 9, 3, base=plain.base, out_col=plain.out_col,
        activation="softmax")
    rng = np.random.Generator(np.random.Philox(key=[59, 7]))
    X = rng.normal(size=(50, 9))
    assert np.array_equal(routed(X), plain(X))
    assert routed.cat_left.shape == (0, 8)
    same = RoutedTreeEnsemblePredictor.random(9, 3, trees=12, depth=4, seed=4,
                                              p_missing_left=0.3)
    assert np.array_equal(same(X), plain(X))         # no NaN: flags are idle
    X[::3, 2] = NAN
    assert np.isfinite(same(X)).all()


# ----------------------------------------------------------------------- #
# torch modules, packed tables

def _mixed_ensemble():
    """Random trees of depth 4 over 9 features, the last two categorical
    (codes), and a chain of exactly 64 splits that alternates numeric and
    categorical nodes: bit 63 of the decision word is in use."""
    rnd = RoutedTreeEnsemblePredictor.random(
        9, 3, trees=5, depth=4, seed=8, n_categorical=2, p_missing_left=0.5)
    rng = np.random.Generator(np.random.Philox(key=[59, 3]))
    n_int = 64
    n_nodes = 2 * n_int + 1
    feat = np.full(n_nodes, -2)
    thr = np.zeros(n_nodes)
    left = np.full(n_nodes, -1)
    right = np.full(n_nodes, -1)
    ml = np.zeros(n_nodes, dtype=bool)
    cr = np.full(n_nodes, -1)
    sets = [row for row in rnd.cat_left]
    for i in range(n_int):
        k = 2 * i
        feat[k] = 7 + (i % 2) if i % 3 == 0 else i % 7
        left[k], right[k] = k + 1, k + 2
        ml[k] = rng.uniform() < 0.5
        thr[k] = np.inf if i % 11 == 5 else rng.normal(-1.0, 0.7)
        if i % 3 == 0:
            # sparse sets, so that walks reach the far end of the chain
            cr[k] = len(sets)
            sets.append(_bitset(rng.choice(256, size=40, replace=False)))
    ml[2 * (n_int - 1)] = True                       # bit 63 on a NaN
    chain = {"feature": feat, "threshold": thr, "left": left, "right": right,
             "value": rng.normal(size=n_nodes), "missing_left": ml, "cat_row": cr}
    return RoutedTreeEnsemblePredictor(
        rnd.trees + [chain], 9, 3, base=rnd.base,
        out_col=list(rnd.out_col) + [2], activation="softmax",
        cat_left=np.stack(sets))


def _mixed_rows(n=160):
    rng = np.random.Generator(np.random.Philox(key=[59, 4]))
    X = rng.normal(size=(n, 9))
    codes = np.array([0.0, 31.0, 32.0, 255.0, 256.0, -1.0, 3.7, NAN, 1e6])
    X[:, 7] = np.where(rng.uniform(size=n) < 0.3, rng.choice(codes, size=n),
                       rng.integers(0, 256, size=n))
    X[:, 8] = np.where(rng.uniform(size=n) < 0.3, rng.choice(codes, size=n),
                       rng.integers(0, 256, size=n))
    X[:, :7] = np.where(rng.uniform(size=(n, 7)) < 0.15, NAN, X[:, :7])
    X[-1] = NAN
    return X


@pytest.mark.parametrize("kind", ["hgbc2", "rfc", "mixed"])
def test_torch_modules_match_the_oracle(kind):
    if kind == "mixed":
        pred, rows = _mixed_ensemble(), _mixed_rows()
    else:
        _, rows, pred = _case(kind)
    want = pred(rows)
    xt = torch.from_numpy(rows)
    with torch.no_grad():
        got32 = pred.torch_module()(xt.float()).double().numpy()
        got64 = pred.build_module(torch.float64)(xt).numpy()
    assert np.allclose(got32, want, rtol=0.0, atol=1e-6), np.abs(got32 - want).max()
    assert np.allclose(got64, want, rtol=0.0, atol=1e-12), np.abs(got64 - want).max()


def _internal_preorder(tr):
    """Internal nodes of one tree in preorder: position = bit index."""
    order, stack = [], [0]
    while stack:
        i = stack.pop()
        if tr["left"][i] >= 0:
            order.append(i)
            stack.append(int(tr["right"][i]))
            stack.append(int(tr["left"][i]))
    return order


def _oracle_bits(pred, X):
    """(rows, T) uint64 decision words from the oracle: node i of a tree is
    asked on its own, as a stump whose left leaf is 1."""
    out = np.zeros((X.shape[0], pred.n_trees), dtype=np.uint64)
    for ti, tr in enumerate(pred.trees):
        for k, i in enumerate(_internal_preorder(tr)):
            one = RoutedTreeEnsemblePredictor(
                [_stump(int(tr["feature"][i]), float(tr["threshold"][i]), 1.0,
                        0.0, bool(tr["missing_left"][i]), int(tr["cat_row"][i]))],
                pred.n_features, 1, cat_left=pred.cat_left,
                categories=pred.categories)
            bit = one.raw(X)[:, 0].astype(np.uint64)
            out[:, ti] |= bit << np.uint64(k)
    return out


@pytest.mark.parametrize("kind", ["hgbc2", "mixed"])
def test_decision_bits_of_a_routed_pack(kind):
    if kind == "mixed":
        pred, rows = _mixed_ensemble(), _mixed_rows()
    else:
        _, rows, pred = _case(kind)
    params = pred.tree_params()
    assert tree_pack.envelope_reason(params) is None
    pack = tree_pack.pack_trees(params, np.arange(pred.n_features), "cpu")
    assert pack["routed"] is True
    got = tree_pack.decision_bits(pack, torch.from_numpy(rows).float())
    want = _oracle_bits(pred, rows)
    assert got.dtype == torch.int64 and tuple(got.shape) == want.shape
    assert np.array_equal(got.numpy().view(np.uint64), want)
    if kind == "mixed":
        # the chain uses all 64 bits and bit 63 goes both ways
        top = (want[:, -1] >> np.uint64(63)) & np.uint64(1)
        assert tree_pack._internal_counts(pred.trees)[-1] == 64
        assert 0 < top.sum() < top.shape[0]
        # pad slots of the smaller trees stay 0, NaN rows included
        n0 = tree_pack._internal_counts(pred.trees)[0]
        assert np.all(want[:, 0] >> np.uint64(n0) == 0)


def test_unrouted_pack_keeps_its_decision_bits():
    plain = TreeEnsemblePredictor.random(9, 3, trees=6, depth=4, seed=2)
    pack = tree_pack.pack_trees(plain.tree_params(), np.arange(9), "cpu")
    assert "routed" not in pack and "missing_left" not in pack
    walk = tree_pack.pack_trees_walk(plain.tree_params(), np.arange(9), "cpu")
    assert "routed" not in walk and "cat_left" not in walk
    rng = np.random.Generator(np.random.Philox(key=[59, 5]))
    X = torch.from_numpy(rng.normal(size=(20, 9))).float()
    assert tree_pack.encode_rows(walk, X) is X


def _indexed(pred):
    """The same trees with distinct integers as leaf values, so that a value
    names the leaf that was reached."""
    trees, off = [], 0
    for tr in pred.trees:
        n = len(tr["left"])
        trees.append(dict(tr, value=np.arange(off, off + n, dtype=np.float64)))
        off += n
    return _rebuild(pred, trees=trees, base=None, scale=1.0, activation="none")


def _decode_walk(pack, X):
    """Walk the routed records in numpy as the module docstring of
    ``ops/tree_pack.py`` lays them out: (rows, T) leaf values."""
    nodes = pack["nodes"].numpy()
    roots = pack["roots"].numpy()
    cat_left = pack["cat_left"].numpy().view(np.uint32)
    thr32 = np.ascontiguousarray(nodes[:, 0]).view(np.float32)
    x32 = tree_pack.encode_rows(pack, torch.from_numpy(X)).numpy()
    assert x32.dtype == np.float32
    out = np.zeros((x32.shape[0], roots.shape[0]))
    for r in range(x32.shape[0]):
        for t, node in enumerate(roots):
            steps = 0
            while nodes[node, 1] >= 0:
                v = x32[r, nodes[node, 1]]
                flags = nodes[node, 2]
                assert flags >> 16 in (0, 1 << 13, 1 << 14, 3 << 13)
                ml = bool(flags & tree_pack.WALK_FLAG_MISSING_LEFT)
                if flags & tree_pack.WALK_FLAG_CATEGORICAL:
                    if 0.0 <= v < 256.0:
                        c = int(v)
                        row = cat_left[nodes[node, 0]]
                        go_left = bool((row[c >> 5] >> np.uint32(c & 31)) & 1)
                    else:
                        go_left = ml
                else:
                    go_left = ml if v != v else bool(v <= thr32[node])
                node = node + 1 if go_left else nodes[node, 3]
                steps += 1
            assert steps <= pack["max_depth"] <= tree_pack.WALK_MAX_DEPTH
            value = nodes[node, 0:1].view(np.float32)[0]
            out[r, t] = value
    return out


@pytest.mark.parametrize("kind", ["hgbc3", "mixed"])
def test_walk_pack_reaches_the_oracles_leaves(kind):
    if kind == "mixed":
        pred, rows = _indexed(_mixed_ensemble()), _mixed_rows(80)
        col_group = np.array([0, 0, 1, 2, 2, 2, 3, 4, 4])
    else:
        _, rows, pred = _case(kind)
        pred, rows = _indexed(pred), rows[::2]
        col_group = np.array([0, 0, 1, 2, 3, 3])
    pack = tree_pack.pack_trees_walk(pred.tree_params(), col_group, "cpu")
    assert pack["routed"] is True
    assert pack["cat_left"].dtype == torch.int32 and pack["cat_left"].shape[1] == 8
    nodes = pack["nodes"].numpy()
    split = nodes[:, 1] >= 0
    assert np.array_equal(nodes[split, 2] & tree_pack.WALK_GROUP_MASK,
                          col_group[nodes[split, 1]])
    assert np.all(nodes[~split, 2] < pred.n_out)        # leaves: no flags
    got = _decode_walk(pack, rows)
    want = np.stack(
        [_rebuild(pred, trees=[tr], n_out=1, out_col=[0], base=None).raw(rows)[:, 0]
         for tr in pred.trees], axis=1)
    assert np.array_equal(got, want)


def test_walk_pack_of_a_forest_without_categories_has_a_bitset_row():
    pred = _case("rfc")[2]
    pack = tree_pack.pack_trees_walk(pred.tree_params(), np.arange(D), "cpu")
    assert tuple(pack["cat_left"].shape) == (1, 8)      # C >= 1 is allocated
    assert pack["categories"] == {}


# ----------------------------------------------------------------------- #
# construction, pickling, loader, refusals

def test_constructor_validation():
    ok = _stump(0, 0.0, 1.0, 2.0)
    sets = np.stack([_bitset([1])])
    RoutedTreeEnsemblePredictor([ok], 2, 1)
    RoutedTreeEnsemblePredictor([dict(ok, cat_row=[0, -1, -1])], 2, 1, cat_left=sets)
    with pytest.raises(ValueError, match="one entry per node"):
        RoutedTreeEnsemblePredictor([dict(ok, missing_left=[True])], 2, 1)
    with pytest.raises(ValueError, match="one entry per node"):
        RoutedTreeEnsemblePredictor([dict(ok, cat_row=[0, -1])], 2, 1, cat_left=sets)
    with pytest.raises(ValueError, match="row of cat_left"):
        RoutedTreeEnsemblePredictor([dict(ok, cat_row=[1, -1, -1])], 2, 1,
                                    cat_left=sets)
    with pytest.raises(ValueError, match="row of cat_left"):
        RoutedTreeEnsemblePredictor([dict(ok, cat_row=[0, -1, -1])], 2, 1)
    with pytest.raises(ValueError, match=r"\(C, 8\) uint32"):
        RoutedTreeEnsemblePredictor([ok], 2, 1, cat_left=np.zeros((1, 4), np.uint32))
    with pytest.raises(ValueError, match=r"\(C, 8\) uint32"):
        RoutedTreeEnsemblePredictor([ok], 2, 1, cat_left=np.zeros((1, 8), np.int64))
    with pytest.raises(ValueError, match="sorted"):
        RoutedTreeEnsemblePredictor([ok], 2, 1, categories={0: [2.0, 1.0]})
    with pytest.raises(ValueError, match="float32"):
        RoutedTreeEnsemblePredictor([ok], 2, 1, categories={0: [0.1, 1.0]})
    with pytest.raises(ValueError, match="out of range"):
        RoutedTreeEnsemblePredictor([ok], 2, 1, categories={2: [1.0]})
    with pytest.raises(ValueError, match=r"finite or \+inf"):
        RoutedTreeEnsemblePredictor([dict(ok, threshold=[-np.inf, 0, 0])], 2, 1)
    with pytest.raises(ValueError, match="finite"):
        RoutedTreeEnsemblePredictor([dict(ok, threshold=[NAN, 0, 0])], 2, 1)
    # the parent keeps refusing +inf
    with pytest.raises(ValueError, match="finite"):
        TreeEnsemblePredictor([dict(ok, threshold=[np.inf, 0, 0])], 2, 1)


def test_tree_params_carry_the_routing():
    pred = _mixed_ensemble()
    params = pred.tree_params()
    assert set(params["routing"]) == {"cat_left", "categories"}
    assert params["routing"]["cat_left"] is pred.cat_left
    assert all("missing_left" in tr and "cat_row" in tr for tr in params["trees"])
    assert "routing" not in TreeEnsemblePredictor.random(3, 2).tree_params()


def test_pickle_round_trip_after_torch_module():
    _, rows, pred = _case("hgbc2")
    want = pred(rows)
    pred.torch_module()
    clone = pickle.loads(pickle.dumps(pred))
    assert isinstance(clone, RoutedTreeEnsemblePredictor)
    assert clone._module is None and clone._flat is None   # caches dropped
    assert np.array_equal(clone(rows), want)
    with torch.no_grad():
        got = clone.torch_module()(torch.from_numpy(rows).float()).double().numpy()
    assert np.allclose(got, want, rtol=0.0, atol=1e-6)
    mod = pickle.loads(pickle.dumps(pred.build_module(torch.float64)))
    with torch.no_grad():
        assert np.allclose(mod(torch.from_numpy(rows)).numpy(), want,
                           rtol=0.0, atol=1e-12)


def test_load_model_wraps_pickled_hist_gradient_boosting(tmp_path):
    from distributedkernelshap_amd.utils import load_model

    est, rows, _ = _case("hgbc2")
    path = tmp_path / "predictor.pkl"
    with open(path, "wb") as f:
        pickle.dump(est, f)
    pred = load_model(str(path))
    assert isinstance(pred, RoutedTreeEnsemblePredictor)
    assert np.allclose(pred(rows), est.predict_proba(rows), rtol=0.0, atol=1e-12)


def test_from_sklearn_refuses_with_reason():
    pytest.importorskip("sklearn")
    from sklearn.ensemble import (GradientBoostingClassifier,
                                  HistGradientBoostingClassifier,
                                  HistGradientBoostingRegressor)
    from sklearn.linear_model import LogisticRegression

    X, y, score = _data(2, n=200)
    X = np.nan_to_num(X)
    pois = HistGradientBoostingRegressor(loss="poisson", max_iter=3).fit(
        X, np.exp(0.2 * score))
    with pytest.raises(TypeError, match="poisson"):
        RoutedTreeEnsemblePredictor.from_sklearn(pois)
    gamma = HistGradientBoostingRegressor(loss="gamma", max_iter=3).fit(
        X, np.exp(0.2 * score))
    with pytest.raises(TypeError, match="gamma"):
        RoutedTreeEnsemblePredictor.from_sklearn(gamma)
    gbc = GradientBoostingClassifier(n_estimators=2).fit(X, y)
    with pytest.raises(TypeError, match=r"TreeEnsemblePredictor\.from_sklearn"):
        RoutedTreeEnsemblePredictor.from_sklearn(gbc)
    with pytest.raises(TypeError, match="LogisticRegression"):
        RoutedTreeEnsemblePredictor.from_sklearn(LogisticRegression().fit(X, y))
    with pytest.raises(TypeError, match="not a sklearn estimator"):
        RoutedTreeEnsemblePredictor.from_sklearn(object())
    # categories that float32 cannot hold: the device lookup would disagree
    X[:, 4] = np.where(X[:, 4] > 2, 0.1, 16777217.0)
    odd = HistGradientBoostingClassifier(
        max_iter=3, categorical_features=[4]).fit(X, y)
    with pytest.raises(TypeError, match="float32"):
        RoutedTreeEnsemblePredictor.from_sklearn(odd)
    # the plain class points at this one
    with pytest.raises(TypeError, match="RoutedTreeEnsemblePredictor"):
        TreeEnsemblePredictor.from_sklearn(odd)


@pytest.mark.parametrize("loss", ["absolute_error", "quantile"])
def test_identity_link_regressor_losses(loss):
    pytest.importorskip("sklearn")
    from sklearn.ensemble import HistGradientBoostingRegressor

    X, _, score = _data(2, n=300)
    kw = {"quantile": 0.7} if loss == "quantile" else {}
    est = HistGradientBoostingRegressor(
        loss=loss, max_iter=5, categorical_features=[4, 5], **kw).fit(X, score)
    pred = RoutedTreeEnsemblePredictor.from_sklearn(est)
    rows = _rows(X)
    assert np.allclose(pred(rows)[:, 0], est.predict(rows), rtol=0.0, atol=1e-12)


def test_cpu_engine_explains_rows_with_nan():
    """The CPU engine blends with a select, so NaN survives; a NaN in x or in
    the background marks its column as varying."""
    from distributedkernelshap_amd.core.engine import KernelShapEngine
    from distributedkernelshap_amd.core.links import logit

    est, rows, pred = _case("hgbc2")
    bg = rows[:20]
    X = np.concatenate([rows[60:62], rows[-8:-6]])
    assert np.isnan(bg).any() and np.isnan(X).any()
    eng = KernelShapEngine(pred, bg, link="logit", seed=0, device="cpu")
    sv = eng.shap_values(X)
    fx = logit(pred(X))
    for o in range(2):
        assert np.isfinite(sv[o]).all()
        total = sv[o].sum(axis=1) + eng.expected_value[o]
        assert np.abs(total - fx[:, o]).max() < 1e-3
