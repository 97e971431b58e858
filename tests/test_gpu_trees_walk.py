"""Fused predict for deep trees (fused_predict_trees_walk) on the GPU: the
kernel against an explicit blend fed to the numpy oracle, and the engine end
to end against the CPU oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from distributedkernelshap_amd.models import TreeEnsemblePredictor  # noqa: E402
from distributedkernelshap_amd.ops import tree_pack  # noqa: E402

A32 = np.float32(0.3)
B32 = np.nextafter(A32, np.float32(np.inf))
# float64 thresholds strictly between the float32 neighbours A32 and B32
THR_HI = float(A32) + 0.75 * (float(B32) - float(A32))
THR_LO = float(A32) + 0.25 * (float(B32) - float(A32))


@pytest.fixture(scope="module")
def ext():
    from distributedkernelshap_amd.ops import load_extension

    return load_extension()


# ----------------------------------------------------------------------- #
# kernel level

def _chunked_groups(d, m):
    cuts = np.linspace(0, d, m + 1).round().astype(int)
    return [list(range(cuts[i], cuts[i + 1])) for i in range(m)]


def _chain(n_internal, feats, rng, sparse=False):
    """Degenerate chain: the right child of every split is the next split,
    the left child a leaf (depth = n_internal). ``sparse`` leaves only one
    split in nine and the last three undecided, so that a good share of the
    walks reaches the far end of a long chain."""
    n_nodes = 2 * n_internal + 1
    feat = np.full(n_nodes, -2)
    thr = np.zeros(n_nodes)
    left = np.full(n_nodes, -1)
    right = np.full(n_nodes, -1)
    for i in range(n_internal):
        feat[2 * i] = feats[i % len(feats)]
        thr[2 * i] = rng.normal(-1.0, 0.7)
        if sparse:
            # every row goes right, except at the few undecided splits
            thr[2 * i] = (rng.normal(-1.2, 0.5)
                          if i % 9 == 4 or i >= n_internal - 3 else -6.0)
        left[2 * i] = 2 * i + 1
        right[2 * i] = 2 * i + 2
    if sparse:
        thr[2 * (n_internal - 1)] = 0.0      # the last split goes both ways
    return {"feature": feat, "threshold": thr, "left": left, "right": right,
            "value": rng.normal(0.0, 1.0, size=n_nodes)}


def _stump(feature, thr, lo, hi):
    return {"feature": [feature, -2, -2], "threshold": [thr, 0.0, 0.0],
            "left": [1, -1, -1], "right": [2, -1, -1], "value": [0.0, lo, hi]}


def _single_leaf(v):
    return {"feature": [-2], "threshold": [0.0], "left": [-1], "right": [-1],
            "value": [v]}


def _exact(pred):
    """The same ensemble with leaves on a 2^-10 grid: every partial sum of
    up to 1024 leaves below 8 in magnitude is exact in fp32, so the raw score
    carries no summation error whatever the number of trees."""
    trees = [dict(t, value=np.round(t["value"] * 1024.0) / 1024.0)
             for t in pred.trees]
    return TreeEnsemblePredictor(
        trees, pred.n_features, pred.n_out, base=pred.base, scale=pred.scale,
        out_col=pred.out_col, activation=pred.activation)


def _internal(pred):
    return tree_pack._internal_counts(pred.trees)


def _shape1_predictor():
    p = TreeEnsemblePredictor.random(7, 1, trees=3, depth=8, p_stop=0.0,
                                     seed=1, activation="sigmoid")
    return TreeEnsemblePredictor(
        p.trees + [_stump(5, 0.2, -0.5, 0.75), _single_leaf(0.3)], 7, 1,
        base=p.base, activation="sigmoid")


def _predictor(shape_id, rng):
    if shape_id == 1:
        return _shape1_predictor()
    if shape_id == 2:
        # exactly 64 splits in a row: the walk's step bound + a stump
        return TreeEnsemblePredictor(
            [_chain(64, list(range(33)), rng, sparse=True),
             _stump(32, 0.1, -0.5, 0.75)],
            33, 8, base=rng.normal(size=8), out_col=[7, 0])
    if shape_id == 3:
        p = TreeEnsemblePredictor.random(9, 3, trees=6, depth=8, seed=3,
                                         activation="none", vector_leaves=True)
        p.scale = 1.0 / 6
        return p
    if shape_id == 4:
        return TreeEnsemblePredictor.random(9, 3, trees=12, depth=8, seed=2,
                                            activation="softmax")
    if shape_id == 5:
        # features 0, 63, 64, 69 lie in varying groups 0, 63, 64, 69 (64 and
        # 69 in the second bitset word); features 70 and 71 belong to groups
        # the table marks as not varying
        feats = [0, 63, 64, 69, 70, 71]
        pad = TreeEnsemblePredictor.random(72, 2, trees=1, depth=8, seed=5,
                                           p_stop=0.0).trees[0]
        trees = [_chain(6, feats, rng), _chain(6, feats[::-1], rng),
                 _stump(70, 0.0, -1.0, 1.0), _stump(64, 0.2, 0.5, -0.5), pad]
        return TreeEnsemblePredictor(trees, 72, 2, out_col=[0, 1, 1, 0, 1],
                                     activation="softmax")
    if shape_id == 6:
        # more than 1024 trees; 1100 x 63 = 69,300 records (index > 65,535)
        return _exact(TreeEnsemblePredictor.random(
            9, 2, trees=1100, depth=5, seed=6, p_stop=0.0, activation="none"))
    if shape_id == 7:
        # shape 1 with every threshold between the float32 neighbours
        p = _shape1_predictor()
        trees = []
        for ti, tr in enumerate(p.trees):
            k = np.arange(len(tr["left"])) + ti
            trees.append(dict(
                tr, threshold=np.where(k % 2 == 0, THR_HI, THR_LO)))
        return TreeEnsemblePredictor(trees, 7, 1, base=p.base,
                                     activation="sigmoid")
    raise KeyError(shape_id)


# (D, groups, N, S, B) — each the smallest shape that breaks one assumption
SHAPES = {
    # trees of 255 splits, N < wave count, S not a tile multiple, unequal groups
    1: (7, [[0], [1, 2], [3], [4, 5, 6]], 3, 70, 1),
    # 64 splits in a row, n_out = 8 with the last column, two sample tiles
    2: (33, [[j] for j in range(33)], 2, 130, 1),
    # vector leaves (forest form)
    3: (9, _chunked_groups(9, 5), 19, 70, 1),
    # scalar leaves over 3 columns, softmax, B = 3 with distinct x
    4: (9, _chunked_groups(9, 5), 19, 70, 3),
    # 72 groups (a second bitset word) and -1 entries
    5: (72, [[j] for j in range(72)], 5, 70, 2),
    # 1100 trees, 69,300 records
    6: (9, _chunked_groups(9, 5), 5, 40, 2),
    # shape 1 on thresholds off the float32 grid
    7: (7, [[0], [1, 2], [3], [4, 5, 6]], 3, 70, 1),
}


def _problem(shape_id):
    d, groups, n, s, b = SHAPES[shape_id]
    # (a key at which the x and background rows of shape 2 fall on both
    # sides of the chain's last split)
    rng = np.random.Generator(np.random.Philox(key=[103, shape_id]))
    pred = _predictor(shape_id, rng)
    x = rng.normal(size=(b, d))
    bg = rng.normal(size=(n, d))
    if shape_id == 7:
        # every entry is one of the two float32 neighbours of the thresholds
        x = np.where(rng.uniform(size=(b, d)) < 0.5, A32, B32).astype(np.float64)
        bg = np.where(rng.uniform(size=(n, d)) < 0.5, A32, B32).astype(np.float64)
    wbg = rng.uniform(0.2, 1.0, size=n)          # non-uniform
    wbg /= wbg.sum()
    col_group = np.empty(d, dtype=np.int64)
    for gi, g in enumerate(groups):
        col_group[g] = gi
    vmap = np.arange(len(groups), dtype=np.int32)
    if shape_id == 5:
        vmap[70:] = -1        # x differs there, yet the background must rule
    m = int((vmap >= 0).sum())
    masks = (rng.uniform(size=(b, s, m)) < 0.5).astype(np.uint8)
    return dict(pred=pred, x=x, bg=bg, wbg=wbg, masks=masks,
                col_group=col_group, vmap=vmap)


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


def _run_kernel(ext, p, pred=None):
    dev = "cuda"
    pred = p["pred"] if pred is None else pred
    pack = tree_pack.pack_trees_walk(pred.tree_params(), p["col_group"], dev)
    x = torch.from_numpy(p["x"]).float().to(dev)
    bg = torch.from_numpy(p["bg"]).float().to(dev)
    masks = torch.from_numpy(p["masks"]).to(dev)
    vmap = torch.from_numpy(p["vmap"]).to(dev)
    wbg = torch.from_numpy(p["wbg"]).float().to(dev)
    b, s, _ = p["masks"].shape
    ey = torch.full((b, s, pred.n_out), float("nan"), device=dev)
    tree_pack.fused_predict_walk(ext, pack, masks, vmap, x, bg, wbg, ey)
    torch.cuda.synchronize()
    return ey.double().cpu().numpy()


@pytest.mark.parametrize("shape_id", sorted(SHAPES))
def test_walk_vs_blend_reference(ext, shape_id):
    """The split decisions are exact, so the only error is the fp32 rounding
    of the leaves and of their sum (shapes 1-5 and 7: at most 12 leaves of
    magnitude ~1; shape 6: exact sums on a 2^-10 leaf grid) and of the N
    weighted terms: the project's fused-predict bounds."""
    p, ref = _ref(shape_id)
    ey = _run_kernel(ext, p)
    assert ey.shape == ref.shape
    err = np.abs(ey - ref).max()
    print(f"shape {shape_id}: fp32 max abs err vs blend reference = {err:.3e}")
    assert np.allclose(ey, ref, atol=2e-5, rtol=1e-4), err


def test_walk_shapes_guard_what_they_claim():
    assert min(_internal(_ref(1)[0]["pred"])[:3]) > 64
    assert max(_internal(_ref(2)[0]["pred"])) == 64
    assert max(_internal(_ref(5)[0]["pred"])) > 64
    p6 = _ref(6)[0]["pred"]
    assert p6.n_trees > 1024
    assert sum(len(t["left"]) for t in p6.trees) == 69300


def test_walk_batch_rows_differ():
    # shape 4 is only a batch-stride guard if the instances really differ
    p, ref = _ref(4)
    assert np.abs(ref[0] - ref[1]).max() > 1e-3
    assert np.abs(ref[1] - ref[2]).max() > 1e-3


def test_walk_chain_is_walked_to_its_end():
    # shape 2 only guards the step bound if walks get there: the share of
    # blended rows that end in one of the last split's leaves
    p, _ = _ref(2)
    chain = p["pred"].trees[0]
    last = np.zeros(len(chain["value"]))
    last[-2:] = 1.0
    share = _reference(dict(p, pred=TreeEnsemblePredictor(
        [dict(chain, value=last)], 33, 1)))
    assert share.mean() > 0.05
    # both of the last split's leaves are reached
    for k in (-2, -1):
        one = np.zeros(len(chain["value"]))
        one[k] = 1.0
        assert _reference(dict(p, pred=TreeEnsemblePredictor(
            [dict(chain, value=one)], 33, 1))).max() > 0.0


def test_walk_nonvarying_groups_matter():
    # shape 5 only guards the -1 entries if treating them as varying would
    # change the answer
    p, ref = _ref(5)
    q = dict(p, vmap=np.arange(72, dtype=np.int32),
             masks=np.concatenate(
                 [p["masks"], np.ones(p["masks"].shape[:2] + (2,), np.uint8)],
                 axis=2))
    assert np.abs(_reference(q) - ref).max() > 1e-3


def test_walk_off_grid_thresholds_matter():
    # shape 7 only guards the threshold rule if thresholds cast to the
    # nearest float32 would change the answer
    p, ref = _ref(7)
    cast = [dict(t, threshold=np.asarray(t["threshold"]).astype(np.float32)
                 .astype(np.float64)) for t in p["pred"].trees]
    q = dict(p, pred=TreeEnsemblePredictor(
        cast, 7, 1, base=p["pred"].base, activation="sigmoid"))
    assert np.abs(_reference(q) - ref).max() > 1e-3


def test_walk_two_launches_identical(ext):
    p, _ = _ref(3)
    assert np.array_equal(_run_kernel(ext, p), _run_kernel(ext, p))
    p, _ = _ref(6)
    assert np.array_equal(_run_kernel(ext, p), _run_kernel(ext, p))


def test_walk_65_splits_in_a_row_raises(ext):
    p, _ = _ref(2)
    rng = np.random.Generator(np.random.Philox(key=[97, 0]))
    deep = TreeEnsemblePredictor([_chain(65, list(range(33)), rng)], 33, 8)
    with pytest.raises(RuntimeError, match="envelope"):
        _run_kernel(ext, p, deep)


def test_walk_n_out_9_raises(ext):
    p, _ = _ref(2)
    wide = TreeEnsemblePredictor([_stump(32, 0.1, -0.5, 0.75)], 33, 9)
    with pytest.raises(RuntimeError, match="envelope"):
        _run_kernel(ext, p, wide)


# ----------------------------------------------------------------------- #
# end to end: d = 8 singleton groups, full enumeration (no sampling noise)

D = 8


def _e2e_data():
    rng = np.random.Generator(np.random.Philox(key=[73, 8]))
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
    pred = TreeEnsemblePredictor.random(D, 2, trees=6, depth=9, p_stop=0.05)
    bg, X = _e2e_data()
    sv_cpu = _engine(pred, bg, "cpu").shap_values(X)
    return pred, bg, X, sv_cpu, _engine(pred, bg, "cuda")


def test_engine_walk_matches_cpu_oracle(e2e):
    from distributedkernelshap_amd.core.links import logit

    pred, bg, X, sv_cpu, gpu = e2e
    assert max(_internal(pred)) > 64
    assert gpu._gpu.trees_fused is True
    assert gpu._gpu.trees_kernel == "walk"
    sv = gpu.shap_values(X)
    fx = logit(pred(X))
    for o in range(2):
        assert sv[o].shape == (4, D)
        assert np.allclose(sv[o], sv_cpu[o], atol=5e-4, rtol=5e-3), \
            np.abs(sv[o] - sv_cpu[o]).max()
        total = sv[o].sum(axis=1) + gpu.expected_value[o]
        assert np.abs(total - fx[:, o]).max() < 1e-3


def test_engine_walk_deterministic_and_split(e2e):
    pred, bg, X, sv_cpu, gpu = e2e
    a = gpu.shap_values(X)
    b = gpu.shap_values(X)
    p1 = gpu.shap_values(X[:2], instance_offset=0)
    p2 = gpu.shap_values(X[2:], instance_offset=2)
    for o in range(2):
        assert np.array_equal(a[o], b[o])
        assert np.allclose(a[o], np.concatenate([p1[o], p2[o]]), atol=1e-5)


def test_walk_on_sample_slice(e2e):
    """The sample-sharded path hands the shared non-linear helper a slice of
    the sample axis: the slice's ey equals the same rows of the full call
    (a sample's arithmetic does not depend on its position in the tile)."""
    pred, bg, X, _, gpu = e2e
    g = gpu._gpu
    assert g.trees_kernel == "walk"
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


def test_engine_walk_mixed_buckets(e2e):
    pred, _, _, _, _ = e2e
    bg, X = _e2e_data()
    bg[:, 3] = 0.7                 # constant background column ...
    X[1, 3] = 0.7                  # ... that instance 1 matches: 7 varying
    sv_cpu = _engine(pred, bg, "cpu").shap_values(X)
    gpu = _engine(pred, bg, "cuda")
    sv = gpu.shap_values(X)
    assert gpu._gpu.trees_kernel == "walk"
    for o in range(2):
        assert sv[o][1, 3] == 0.0
        assert np.allclose(sv[o], sv_cpu[o], atol=5e-4, rtol=5e-3), \
            np.abs(sv[o] - sv_cpu[o]).max()


def test_engine_walk_fp64_mode_matches_cpu_oracle(e2e):
    pred, bg, X, sv_cpu, _ = e2e
    gpu = _engine(pred, bg, "cuda", predict_dtype="fp64")
    sv = gpu.shap_values(X)
    for o in range(2):
        assert np.allclose(sv[o], sv_cpu[o], rtol=0.0, atol=1e-8), \
            np.abs(sv[o] - sv_cpu[o]).max()


def test_engine_shallow_trees_keep_the_bit_register_kernel():
    pred = TreeEnsemblePredictor.random(D, 2, trees=6, depth=3, seed=11)
    bg, _ = _e2e_data()
    gpu = _engine(pred, bg, "cuda")
    assert gpu._gpu.trees_fused is True
    assert gpu._gpu.trees_kernel == "bits"


def test_kernel_shap_public_api_sklearn_random_forest():
    from sklearn.ensemble import RandomForestClassifier

    from distributedkernelshap_amd import KernelShap
    from distributedkernelshap_amd.core.links import logit
    from distributedkernelshap_amd.models import make_adult_like

    data = make_adult_like(n_instances=8, n_background=25)
    train = make_adult_like(n_instances=600, n_background=1, seed=3).X
    y = (train[:, 0] + train[:, 1] * train[:, 2] > np.median(train[:, 0])).astype(int)
    est = RandomForestClassifier(n_estimators=10, random_state=0).fit(train, y)
    pred = TreeEnsemblePredictor.from_sklearn(est)
    assert max(_internal(pred)) > 64
    ks = KernelShap(pred, link="logit", device="cuda")
    ks.fit(data.background, groups=data.groups, group_names=data.group_names)
    assert ks._explainer._engine._gpu.trees_kernel == "walk"
    exp = ks.explain(data.X)
    sv = exp.shap_values
    fx = logit(pred(data.X))
    assert len(sv) == 2
    for o in range(2):
        assert sv[o].shape == (8, 12)
        assert np.isfinite(sv[o]).all()
        total = sv[o].sum(axis=1) + ks.expected_value[o]
        assert np.abs(total - fx[:, o]).max() < 1e-3
