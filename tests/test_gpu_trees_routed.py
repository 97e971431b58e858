"""Routed tree ensembles (missing values, categorical splits) on the GPU: the
routed walk kernel and the bit-register kernel on a routed pack against an
explicit blend fed to the numpy oracle, and the engine end to end on fitted
HistGradientBoosting models against the CPU oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from distributedkernelshap_amd.models import (  # noqa: E402
    RoutedTreeEnsemblePredictor,
    TreeEnsemblePredictor,
)
from distributedkernelshap_amd.ops import tree_pack  # noqa: E402

NAN = float("nan")
# raw values of the categorical feature that carries a category table: 40
# known values, none of them contiguous
KNOWN = 3.0 + 2.0 * np.arange(40.0)
# codes / raw values at the edges of the rule
EDGE_CODES = np.array([0.0, 31.0, 32.0, 255.0, 256.0, 300.0, -1.0, -0.5, 3.7,
                       254.9, NAN])
EDGE_RAW = np.array([3.0, 65.0, 67.0, 81.0, 4.0, 0.0, -3.0, 1000.0, 3.5, NAN])


@pytest.fixture(scope="module")
def ext():
    from distributedkernelshap_amd.ops import load_extension

    return load_extension()


# ----------------------------------------------------------------------- #
# kernel level

def _chunked_groups(d, m):
    cuts = np.linspace(0, d, m + 1).round().astype(int)
    return [list(range(cuts[i], cuts[i + 1])) for i in range(m)]


def _rebuild(pred, **kw):
    args = dict(trees=pred.trees, n_features=pred.n_features, n_out=pred.n_out,
                base=pred.base, scale=pred.scale, out_col=pred.out_col,
                activation=pred.activation, cat_left=pred.cat_left,
                categories=pred.categories)
    args.update(kw)
    return RoutedTreeEnsemblePredictor(**args)


def _bitset(codes):
    row = np.zeros(8, dtype=np.uint32)
    for c in codes:
        row[c >> 5] |= np.uint32(1) << np.uint32(c & 31)
    return row


def _routed_chain(n_internal, feats, cat_feats, rng, first_row):
    """The right child of every split is the next split, the left a leaf;
    splits on ``cat_feats`` are categorical with half of the codes left."""
    n_nodes = 2 * n_internal + 1
    feat = np.full(n_nodes, -2)
    thr = np.zeros(n_nodes)
    left = np.full(n_nodes, -1)
    right = np.full(n_nodes, -1)
    ml = np.zeros(n_nodes, dtype=bool)
    cr = np.full(n_nodes, -1)
    sets = []
    for i in range(n_internal):
        k = 2 * i
        feat[k] = feats[i % len(feats)]
        thr[k] = rng.normal(-0.5, 0.7)
        left[k], right[k] = k + 1, k + 2
        ml[k] = rng.uniform() < 0.5
        if feat[k] in cat_feats:
            cr[k] = first_row + len(sets)
            sets.append(_bitset(rng.choice(256, size=128, replace=False)))
    tree = {"feature": feat, "threshold": thr, "left": left, "right": right,
            "value": rng.normal(0.0, 1.0, size=n_nodes), "missing_left": ml,
            "cat_row": cr}
    return tree, sets


def _predictor(shape_id, depth, rng):
    if shape_id in (1, 3):
        p = RoutedTreeEnsemblePredictor.random(
            7, 1, trees=3, depth=depth, p_stop=0.0, seed=1,
            activation="sigmoid", p_missing_left=0.5)
        if shape_id == 1:
            return p
        # a third of the thresholds: "every non-missing value goes left"
        trees = []
        for ti, tr in enumerate(p.trees):
            k = np.arange(len(tr["left"])) + ti
            trees.append(dict(tr, threshold=np.where(
                (k % 3 == 0) & (tr["left"] >= 0), np.inf, tr["threshold"])))
        return _rebuild(p, trees=trees)
    if shape_id == 2:
        # features 7 (raw values looked up in KNOWN) and 8 (codes) categorical
        p = RoutedTreeEnsemblePredictor.random(
            9, 2, trees=12, depth=depth, seed=2, activation="softmax",
            n_categorical=2)
        return _rebuild(p, categories={7: KNOWN})
    if shape_id == 4:
        # features 0, 63, 64, 69 lie in varying groups (64 and 69 in the
        # second bitset word); 70 and 71 in groups marked as not varying;
        # 64 and 71 are categorical
        feats = [0, 63, 64, 69, 70, 71]
        pad = RoutedTreeEnsemblePredictor.random(
            72, 2, trees=1, depth=depth, seed=5, p_stop=0.0)
        pad_tree = pad.trees[0]
        c1, s1 = _routed_chain(6, feats, (64, 71), rng, 0)
        c2, s2 = _routed_chain(6, feats[::-1], (64, 71), rng, len(s1))
        return RoutedTreeEnsemblePredictor(
            [c1, c2, pad_tree], 72, 2, out_col=[0, 1, 1], activation="softmax",
            cat_left=np.stack(s1 + s2))
    if shape_id == 5:
        p = RoutedTreeEnsemblePredictor.random(
            9, 8, trees=6, depth=depth, seed=3, activation="none",
            vector_leaves=True, n_categorical=2)
        p.scale = 1.0 / 6
        return p
    if shape_id == 6:
        # all flags clear, no categorical split: the plain forest's tables
        plain = TreeEnsemblePredictor.random(9, 3, trees=12, depth=depth, seed=2,
                                             activation="softmax")
        return RoutedTreeEnsemblePredictor(
            plain.trees, 9, 3, base=plain.base, out_col=plain.out_col,
            activation="softmax")
    raise KeyError(shape_id)


# (D, groups, N, S, B) — each the smallest shape that breaks one assumption
SHAPES = {
    # trees of 255 splits with random missing_left, NaN in x and background,
    # N < wave count, S not a tile multiple, unequal groups
    1: (7, [[0], [1, 2], [3], [4, 5, 6]], 3, 70, 1),
    # two categorical features, every edge of the code range, B = 3
    2: (9, _chunked_groups(9, 5), 19, 70, 3),
    # shape 1 with +inf thresholds
    3: (7, [[0], [1, 2], [3], [4, 5, 6]], 3, 70, 1),
    # 72 groups (a second bitset word), -1 entries, background in global
    # memory: 4 B x 72 x 300 > 80 KiB
    4: (72, [[j] for j in range(72)], 300, 70, 2),
    # vector leaves, n_out = 8
    5: (9, _chunked_groups(9, 5), 19, 70, 1),
    # flags clear, no NaN: must equal the unrouted kernel bit for bit
    6: (9, _chunked_groups(9, 5), 19, 70, 3),
}
CAT_CODE_COLS = {2: [8], 4: [64, 71], 5: [7, 8]}       # columns holding codes


def _sprinkle(rng, a, values, share):
    """Replace a share of the entries of the 1-d array ``a`` by edge values."""
    hit = rng.uniform(size=a.shape) < share
    return np.where(hit, rng.choice(values, size=a.shape), a)


def _problem(shape_id, depth=8):
    d, groups, n, s, b = SHAPES[shape_id]
    rng = np.random.Generator(np.random.Philox(key=[107, shape_id]))
    pred = _predictor(shape_id, depth, rng)
    x = rng.normal(size=(b, d))
    bg = rng.normal(size=(n, d))
    if shape_id != 6:
        # NaN in x and in some background entries (the categorical
        # columns get theirs with the edge values below)
        x = np.where(rng.uniform(size=x.shape) < 0.25, NAN, x)
        bg = np.where(rng.uniform(size=bg.shape) < 0.15, NAN, bg)
        x[0, 0] = bg[0, 1] = NAN                  # whatever the draw
    for col in CAT_CODE_COLS.get(shape_id, []):
        x[:, col] = _sprinkle(rng, rng.integers(0, 256, size=b).astype(float),
                              EDGE_CODES, 0.5)
        bg[:, col] = _sprinkle(rng, rng.integers(0, 256, size=n).astype(float),
                               EDGE_CODES, 0.5)
    if shape_id == 2:
        # every edge appears in the background whatever the draw
        bg[:len(EDGE_CODES), 8] = EDGE_CODES
        x[:, 7] = [EDGE_RAW[4], KNOWN[31], NAN]         # unknown, known, NaN
        bg[:, 7] = _sprinkle(rng, rng.choice(KNOWN, size=n), EDGE_RAW, 0.4)
        bg[:len(EDGE_RAW), 7] = EDGE_RAW
    wbg = rng.uniform(0.2, 1.0, size=n)          # non-uniform
    wbg /= wbg.sum()
    col_group = np.empty(d, dtype=np.int64)
    for gi, g in enumerate(groups):
        col_group[g] = gi
    vmap = np.arange(len(groups), dtype=np.int32)
    if shape_id == 4:
        vmap[70:] = -1        # x differs there, yet the background must rule
    m = int((vmap >= 0).sum())
    masks = (rng.uniform(size=(b, s, m)) < 0.5).astype(np.uint8)
    return dict(pred=pred, x=x, bg=bg, wbg=wbg, masks=masks,
                col_group=col_group, vmap=vmap)


def _reference(p):
    """Explicit (B, S, N, D) blend fed to the numpy oracle (NaN survives the
    select)."""
    b, s, _ = p["masks"].shape
    n, d = p["bg"].shape
    colv = p["vmap"][p["col_group"]]                           # (D,)
    on = np.where(colv >= 0, p["masks"][:, :, np.maximum(colv, 0)], 0) != 0
    rows = np.where(on[:, :, None, :], p["x"][:, None, None, :],
                    p["bg"][None, None, :, :])
    pr = p["pred"](rows.reshape(-1, d)).reshape(b, s, n, -1)
    return np.einsum("bsno,n->bso", pr, p["wbg"])


_REF = {}


def _ref(shape_id, depth=8):
    """Problem + reference, computed once and shared (never mutated)."""
    if (shape_id, depth) not in _REF:
        p = _problem(shape_id, depth)
        _REF[shape_id, depth] = (p, _reference(p))
    return _REF[shape_id, depth]


def _operands(p):
    dev = "cuda"
    b, s, _ = p["masks"].shape
    return dict(
        x=torch.from_numpy(p["x"]).float().to(dev),
        bg=torch.from_numpy(p["bg"]).float().to(dev),
        masks=torch.from_numpy(p["masks"]).to(dev),
        vmap=torch.from_numpy(p["vmap"]).to(dev),
        wbg=torch.from_numpy(p["wbg"]).float().to(dev), b=b, s=s)


def _run_walk(ext, p, pred=None):
    pred = p["pred"] if pred is None else pred
    o = _operands(p)
    pack = tree_pack.pack_trees_walk(pred.tree_params(), p["col_group"], "cuda")
    ey = torch.full((o["b"], o["s"], pred.n_out), NAN, device="cuda")
    tree_pack.fused_predict_walk(
        ext, pack, o["masks"], o["vmap"], tree_pack.encode_rows(pack, o["x"]),
        tree_pack.encode_rows(pack, o["bg"]), o["wbg"], ey)
    torch.cuda.synchronize()
    return ey


def _run_bits(ext, p):
    pred = p["pred"]
    o = _operands(p)
    pack = tree_pack.pack_trees(pred.tree_params(), p["col_group"], "cuda")
    dx = tree_pack.decision_bits(pack, o["x"])
    dbg = tree_pack.decision_bits(pack, o["bg"])
    ey = torch.full((o["b"], o["s"], pred.n_out), NAN, device="cuda")
    tree_pack.fused_predict(ext, pack, o["masks"], o["vmap"], dx, dbg,
                            o["wbg"], ey)
    torch.cuda.synchronize()
    return ey


def _internal(pred):
    return tree_pack._internal_counts(pred.trees)


@pytest.mark.parametrize("shape_id", sorted(SHAPES))
def test_routed_walk_vs_blend_reference(ext, shape_id):
    """The routing decisions are exact, so the only error is the fp32
    rounding of at most 12 leaves of magnitude ~1 and of the N weighted
    terms: the project's fused-predict bounds."""
    p, ref = _ref(shape_id)
    assert np.isfinite(ref).all()
    ey = _run_walk(ext, p).double().cpu().numpy()
    assert ey.shape == ref.shape
    err = np.abs(ey - ref).max()
    print(f"shape {shape_id}: fp32 max abs err vs blend reference = {err:.3e}")
    assert np.allclose(ey, ref, atol=2e-5, rtol=1e-4), err


@pytest.mark.parametrize("shape_id", [1, 2])
def test_bit_register_kernel_on_a_routed_pack(ext, shape_id):
    """Trees of depth 4 (at most 15 splits): the routing is in
    ``decision_bits``, the kernel is the unrouted one."""
    p, ref = _ref(shape_id, depth=4)
    assert max(_internal(p["pred"])) <= 64
    assert tree_pack.envelope_reason(p["pred"].tree_params()) is None
    ey = _run_bits(ext, p).double().cpu().numpy()
    err = np.abs(ey - ref).max()
    print(f"shape {shape_id} (bits): max abs err vs blend reference = {err:.3e}")
    assert np.allclose(ey, ref, atol=2e-5, rtol=1e-4), err


def test_routed_walk_with_flags_clear_equals_the_unrouted_kernel(ext):
    p, ref = _ref(6)
    routed = p["pred"]
    assert not np.isnan(p["x"]).any() and not np.isnan(p["bg"]).any()
    assert not any(tr["missing_left"].any() or (tr["cat_row"] >= 0).any()
                   for tr in routed.trees)
    plain = TreeEnsemblePredictor(
        routed.trees, 9, 3, base=routed.base, out_col=routed.out_col,
        activation="softmax")
    assert "routing" not in plain.tree_params()
    assert torch.equal(_run_walk(ext, p), _run_walk(ext, p, plain))


def _flip_missing(pred):
    return _rebuild(pred, trees=[dict(tr, missing_left=~tr["missing_left"])
                                 for tr in pred.trees])


def test_routed_shapes_guard_what_they_claim():
    for shape_id in (1, 2, 3, 4, 5):
        p, ref = _ref(shape_id)
        pred = p["pred"]
        assert max(_internal(pred)) > 64, shape_id
        assert np.isnan(p["x"]).any() and np.isnan(p["bg"]).any()
        # the missing_left flags decide: all of them flipped is another answer
        flipped = _reference(dict(p, pred=_flip_missing(pred)))
        assert np.abs(flipped - ref).max() > 1e-3, shape_id
    assert min(_internal(_ref(1)[0]["pred"])) > 64
    p3 = _ref(3)[0]["pred"]
    assert sum(int(np.isinf(tr["threshold"]).sum()) for tr in p3.trees) > 60
    d, _, n, _, _ = SHAPES[4]
    assert 4 * d * n > 80 * 1024                  # background stays global
    assert len(SHAPES[4][1]) > 64                 # second bitset word
    assert _ref(5)[0]["pred"].vector_leaves and _ref(5)[0]["pred"].n_out == 8


def test_routed_categorical_edges_matter():
    p, ref = _ref(2)
    pred = p["pred"]
    assert sum(int((tr["cat_row"] >= 0).sum()) for tr in pred.trees) > 20
    # every edge of the rule is among the rows
    for v in EDGE_CODES[~np.isnan(EDGE_CODES)]:
        assert (p["bg"][:, 8] == v).any()
    enc = pred.encode(p["bg"])
    assert {0.0, 31.0, 32.0, 39.0} <= set(enc[:, 7][~np.isnan(enc[:, 7])])
    assert np.isnan(enc[:, 7]).sum() >= 7          # unknown raw values -> NaN
    # unknown raw values treated as a known category: another answer
    known = dict(p, x=p["x"].copy(), bg=p["bg"].copy())
    for a in (known["x"], known["bg"]):
        unknown = ~np.isin(a[:, 7], KNOWN)
        a[unknown, 7] = KNOWN[5]
    assert np.abs(_reference(known) - ref).max() > 1e-3
    # codes outside [0, 256) clamped into it instead of routed as missing
    clamped = dict(p, x=p["x"].copy(), bg=p["bg"].copy())
    for a in (clamped["x"], clamped["bg"]):
        a[:, 8] = np.where(np.isnan(a[:, 8]), NAN, np.clip(a[:, 8], 0.0, 255.0))
    assert np.abs(_reference(clamped) - ref).max() > 1e-3
    # fractional codes rounded to nearest instead of truncated
    rounded = dict(p, x=p["x"].copy(), bg=p["bg"].copy())
    for a in (rounded["x"], rounded["bg"]):
        frac = (a[:, 8] > 0) & (a[:, 8] < 255)
        a[frac, 8] = np.round(a[frac, 8])
    assert np.abs(_reference(rounded) - ref).max() > 1e-4


def test_routed_batch_rows_differ():
    # shape 2 is only a batch-stride guard if the instances really differ
    p, ref = _ref(2)
    assert np.abs(ref[0] - ref[1]).max() > 1e-3
    assert np.abs(ref[1] - ref[2]).max() > 1e-3


def test_routed_nonvarying_groups_matter():
    # shape 4 only guards the -1 entries if treating them as varying would
    # change the answer
    p, ref = _ref(4)
    q = dict(p, vmap=np.arange(72, dtype=np.int32),
             masks=np.concatenate(
                 [p["masks"], np.ones(p["masks"].shape[:2] + (2,), np.uint8)],
                 axis=2))
    assert np.abs(_reference(q) - ref).max() > 1e-3


def test_routed_walk_two_launches_identical(ext):
    for shape_id in (2, 4):
        p, _ = _ref(shape_id)
        assert torch.equal(_run_walk(ext, p), _run_walk(ext, p))


def test_routed_walk_65_splits_in_a_row_raises(ext):
    p, _ = _ref(1)
    rng = np.random.Generator(np.random.Philox(key=[107, 0]))
    chain, _ = _routed_chain(65, list(range(7)), (), rng, 0)
    deep = RoutedTreeEnsemblePredictor([chain], 7, 1)
    with pytest.raises(RuntimeError, match="envelope"):
        _run_walk(ext, p, deep)


def test_routed_walk_n_out_9_raises(ext):
    p, _ = _ref(1)
    rng = np.random.Generator(np.random.Philox(key=[107, 9]))
    chain, _ = _routed_chain(3, list(range(7)), (), rng, 0)
    wide = RoutedTreeEnsemblePredictor([chain], 7, 9)
    with pytest.raises(RuntimeError, match="envelope"):
        _run_walk(ext, p, wide)


# ----------------------------------------------------------------------- #
# end to end: fitted HistGradientBoosting, d = 8 singleton groups, full
# enumeration (no sampling noise)

D = 8
CATS = np.array([2.0, 5.0, 9.0, 14.0, 30.0, 77.0])


def _e2e_data():
    """Training rows, 30 background rows and 4 instances: column 6 is
    categorical, column 1 has NaNs (in training, background and instances)."""
    rng = np.random.Generator(np.random.Philox(key=[79, 8]))
    n = 3000
    X = rng.normal(size=(n, D)).astype(np.float32).astype(np.float64)
    X[:, 6] = rng.choice(CATS, size=n)
    score = (X[:, 0] + 0.5 * X[:, 2] * X[:, 3] - X[:, 4]
             + 1.2 * np.isin(X[:, 6], [5.0, 30.0]) + 0.3 * np.sin(3 * X[:, 5]))
    gone = rng.uniform(size=n) < 0.2
    X[gone, 1] = NAN
    score[gone] += 0.7
    score[~gone] += 0.4 * X[~gone, 1]
    y = (score + 0.3 * rng.normal(size=n) > 0.4).astype(int)
    bg = X[:30].copy()
    inst = X[30:34].copy()
    inst[0, 1] = NAN
    inst[1, 6] = 6.0               # a category the model has not seen
    inst[2, 1] = 0.25
    bg[0, 1], bg[1, 1] = NAN, 0.5  # both kinds whatever the draw
    return X[34:], y[34:], bg, inst


def _engine(pred, bg, device, **kernel_kw):
    from distributedkernelshap_amd.config import KernelConfig
    from distributedkernelshap_amd.core.engine import KernelShapEngine

    return KernelShapEngine(
        pred, bg, link="logit", seed=0, device=device,
        kernels=KernelConfig(**kernel_kw) if kernel_kw else None,
    )


_E2E = {}


def _e2e(kind):
    """Predictor, data, CPU-oracle values and one fused GPU engine."""
    if kind not in _E2E:
        pytest.importorskip("sklearn")
        from sklearn.ensemble import HistGradientBoostingClassifier

        Xtr, ytr, bg, X = _e2e_data()
        kw = ({} if kind == "bits"
              else {"max_leaf_nodes": 200, "min_samples_leaf": 3})
        est = HistGradientBoostingClassifier(
            max_iter=12, categorical_features=[6], random_state=0, **kw
        ).fit(Xtr, ytr)
        pred = RoutedTreeEnsemblePredictor.from_sklearn(est)
        assert np.allclose(pred(X), est.predict_proba(X), rtol=0.0, atol=1e-12)
        sv_cpu = _engine(pred, bg, "cpu").shap_values(X)
        _E2E[kind] = (pred, bg, X, sv_cpu, _engine(pred, bg, "cuda"))
    return _E2E[kind]


@pytest.mark.parametrize("kind", ["bits", "walk"])
def test_engine_routed_matches_cpu_oracle(kind):
    from distributedkernelshap_amd.core.links import logit

    pred, bg, X, sv_cpu, gpu = _e2e(kind)
    assert np.isnan(X[:, 1]).any() and np.isnan(bg[:, 1]).any()
    assert any((tr["cat_row"] >= 0).any() for tr in pred.trees)
    assert any(tr["missing_left"].any() for tr in pred.trees)
    if kind == "bits":
        assert max(_internal(pred)) <= 30          # the default 31 leaves
    else:
        assert max(_internal(pred)) > 64
    assert gpu._gpu.trees_fused is True
    assert gpu._gpu.trees_kernel == kind
    sv = gpu.shap_values(X)
    fx = logit(pred(X))
    for o in range(2):
        assert sv[o].shape == (4, D)
        assert np.isfinite(sv[o]).all()
        assert np.allclose(sv[o], sv_cpu[o], atol=5e-4, rtol=5e-3), \
            np.abs(sv[o] - sv_cpu[o]).max()
        total = sv[o].sum(axis=1) + gpu.expected_value[o]
        assert np.abs(total - fx[:, o]).max() < 1e-3
    # the NaN column and the categorical column carry attribution
    assert np.abs(sv[1][:, 1]).max() > 1e-3
    assert np.abs(sv[1][:, 6]).max() > 1e-3
    again = gpu.shap_values(X)
    for o in range(2):
        assert np.array_equal(sv[o], again[o])


@pytest.mark.parametrize("kind", ["bits", "walk"])
def test_engine_routed_fp64_mode_matches_cpu_oracle(kind):
    pred, bg, X, sv_cpu, _ = _e2e(kind)
    gpu = _engine(pred, bg, "cuda", predict_dtype="fp64")
    sv = gpu.shap_values(X)
    for o in range(2):
        assert np.allclose(sv[o], sv_cpu[o], rtol=0.0, atol=1e-8), \
            np.abs(sv[o] - sv_cpu[o]).max()


def test_engine_routed_module_path_when_fused_predict_is_off():
    pred, bg, X, sv_cpu, _ = _e2e("bits")
    gpu = _engine(pred, bg, "cuda", fused_predict=False)
    assert gpu._gpu.trees_fused is False and gpu._gpu.trees_kernel is None
    sv = gpu.shap_values(X)
    for o in range(2):
        assert np.allclose(sv[o], sv_cpu[o], atol=5e-4, rtol=5e-3), \
            np.abs(sv[o] - sv_cpu[o]).max()
