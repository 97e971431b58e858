"""Fused tree predict (fused_predict_trees) on the GPU: the kernel against an
explicit blend fed to the numpy oracle, and the engine end to end against the
CPU oracle."""
import logging

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from distributedkernelshap_amd.models import TreeEnsemblePredictor  # noqa: E402
from distributedkernelshap_amd.ops import tree_pack  # noqa: E402


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


def _exact(pred):
    """The same ensemble with leaves on a 2^-10 grid: every partial sum of
    up to 1024 leaves below 8 in magnitude is exact in fp32, so the raw score
    carries no summation error whatever the number of trees."""
    trees = [dict(t, value=np.round(t["value"] * 1024.0) / 1024.0)
             for t in pred.trees]
    return TreeEnsemblePredictor(
        trees, pred.n_features, pred.n_out, base=pred.base, scale=pred.scale,
        out_col=pred.out_col, activation=pred.activation)


def _predictor(shape_id, rng):
    if shape_id == 1:
        return TreeEnsemblePredictor.random(7, 1, trees=5, depth=2, seed=1,
                                            activation="sigmoid")
    if shape_id in (2, 5):
        return TreeEnsemblePredictor.random(9, 3, trees=12, depth=3, seed=2,
                                            activation="softmax")
    if shape_id == 3:
        p = TreeEnsemblePredictor.random(9, 3, trees=6, depth=3, seed=3,
                                         activation="none", vector_leaves=True)
        p.scale = 1.0 / 6
        return p
    if shape_id == 4:
        # exactly 64 internal nodes (bit 63, leaf codes up to 64 + 64) + a stump
        return TreeEnsemblePredictor(
            [_chain(64, list(range(33)), rng, sparse=True),
             _stump(32, 0.1, -0.5, 0.75)],
            33, 8, base=rng.normal(size=8), out_col=[7, 0])
    if shape_id == 6:
        # features 0, 63, 64, 69 lie in varying groups 0, 63, 64, 69; features
        # 70 and 71 belong to groups the table marks as not varying
        feats = [0, 63, 64, 69, 70, 71]
        trees = [_chain(6, feats, rng), _chain(6, feats[::-1], rng),
                 _stump(70, 0.0, -1.0, 1.0), _stump(64, 0.2, 0.5, -0.5)]
        return TreeEnsemblePredictor(trees, 72, 2, out_col=[0, 1, 1, 0],
                                     activation="softmax")
    if shape_id == 7:       # nm needs the 32-sample tile
        return _exact(TreeEnsemblePredictor.random(
            9, 3, trees=200, depth=2, seed=7, activation="none"))
    if shape_id == 8:       # more than 512 trees: the 16-sample tile
        return _exact(TreeEnsemblePredictor.random(
            9, 2, trees=520, depth=2, seed=8, activation="none",
            vector_leaves=True))
    if shape_id == 9:       # 1000 trees: leaves no longer fit LDS
        return _exact(TreeEnsemblePredictor.random(
            9, 2, trees=1000, depth=3, seed=9, activation="none", p_stop=0.0))
    raise KeyError(shape_id)


# (D, groups, N, S, B) — each the smallest shape that breaks one assumption
SHAPES = {
    # N < wave count, S not a tile multiple, unequal groups
    1: (7, [[0], [1, 2], [3], [4, 5, 6]], 3, 70, 1),
    # scalar leaves spread over 3 output columns, softmax
    2: (9, _chunked_groups(9, 5), 19, 70, 1),
    # vector leaves (forest form)
    3: (9, _chunked_groups(9, 5), 19, 70, 1),
    # 64 internal nodes in one tree, n_out = 8, two sample tiles
    4: (33, [[j] for j in range(33)], 2, 130, 1),
    # B = 3 with distinct x per instance: the batch stride
    5: (9, _chunked_groups(9, 5), 19, 70, 3),
    # 70 varying groups (beyond one 64-bit word of mask bits) and -1 entries
    6: (72, [[j] for j in range(72)], 5, 70, 2),
    # tree counts at which the kernel changes its sample tile / leaf storage
    7: (9, _chunked_groups(9, 5), 5, 40, 2),
    8: (9, _chunked_groups(9, 5), 5, 40, 2),
    9: (9, _chunked_groups(9, 5), 5, 40, 2),
}


def _problem(shape_id):
    d, groups, n, s, b = SHAPES[shape_id]
    rng = np.random.Generator(np.random.Philox(key=[67, shape_id]))
    pred = _predictor(shape_id, rng)
    x = rng.normal(size=(b, d))
    bg = rng.normal(size=(n, d))
    wbg = rng.uniform(0.2, 1.0, size=n)          # non-uniform
    wbg /= wbg.sum()
    col_group = np.empty(d, dtype=np.int64)
    for gi, g in enumerate(groups):
        col_group[g] = gi
    vmap = np.arange(len(groups), dtype=np.int32)
    if shape_id == 6:
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
    pack = tree_pack.pack_trees(pred.tree_params(), p["col_group"], dev)
    dx = tree_pack.decision_bits(pack, torch.from_numpy(p["x"]).to(dev))
    dbg = tree_pack.decision_bits(pack, torch.from_numpy(p["bg"]).to(dev))
    masks = torch.from_numpy(p["masks"]).to(dev)
    vmap = torch.from_numpy(p["vmap"]).to(dev)
    wbg = torch.from_numpy(p["wbg"]).float().to(dev)
    b, s, _ = p["masks"].shape
    ey = torch.full((b, s, pred.n_out), float("nan"), device=dev)
    tree_pack.fused_predict(ext, pack, masks, vmap, dx, dbg, wbg, ey)
    torch.cuda.synchronize()
    return ey.double().cpu().numpy()


@pytest.mark.parametrize("shape_id", sorted(SHAPES))
def test_fused_trees_vs_blend_reference(ext, shape_id):
    """The split decisions are exact, so the only error is the fp32 rounding
    of the leaves and of their sum (shapes 1-6: at most 66 leaves of
    magnitude ~1; shapes 7-9: exact sums on a 2^-10 leaf grid) and of the N
    weighted terms: the project's fused-predict bounds."""
    p, ref = _ref(shape_id)
    ey = _run_kernel(ext, p)
    assert ey.shape == ref.shape
    err = np.abs(ey - ref).max()
    print(f"shape {shape_id}: fp32 max abs err vs blend reference = {err:.3e}")
    assert np.allclose(ey, ref, atol=2e-5, rtol=1e-4), err


def test_fused_trees_batch_rows_differ(ext):
    # shape 5 is only a batch-stride guard if the instances really differ
    p, ref = _ref(5)
    assert np.abs(ref[0] - ref[1]).max() > 1e-3
    assert np.abs(ref[1] - ref[2]).max() > 1e-3


def test_fused_trees_chain_is_walked_to_its_end(ext):
    # shape 4 only guards bit 63 and the last leaf codes if walks get there:
    # the share of blended rows that end in one of the last split's leaves
    p, _ = _ref(4)
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


def test_fused_trees_nonvarying_groups_matter(ext):
    # shape 6 only guards the -1 entries if treating them as varying would
    # change the answer
    p, ref = _ref(6)
    q = dict(p, vmap=np.arange(72, dtype=np.int32),
             masks=np.concatenate(
                 [p["masks"], np.ones(p["masks"].shape[:2] + (2,), np.uint8)],
                 axis=2))
    assert np.abs(_reference(q) - ref).max() > 1e-3


def test_fused_trees_two_launches_identical(ext):
    p, _ = _ref(2)
    assert np.array_equal(_run_kernel(ext, p), _run_kernel(ext, p))
    p, _ = _ref(8)
    assert np.array_equal(_run_kernel(ext, p), _run_kernel(ext, p))


def test_fused_trees_65_internal_nodes_raises(ext):
    p, _ = _ref(4)
    rng = np.random.Generator(np.random.Philox(key=[71, 0]))
    deep = TreeEnsemblePredictor([_chain(65, list(range(33)), rng)], 33, 8)
    with pytest.raises(RuntimeError, match="envelope"):
        _run_kernel(ext, p, deep)


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
    pred = TreeEnsemblePredictor.random(D, 2, trees=20, depth=3)
    bg, X = _e2e_data()
    sv_cpu = _engine(pred, bg, "cpu").shap_values(X)
    return pred, bg, X, sv_cpu, _engine(pred, bg, "cuda")


def test_engine_fused_trees_matches_cpu_oracle(e2e):
    from distributedkernelshap_amd.core.links import logit

    pred, bg, X, sv_cpu, gpu = e2e
    assert gpu._gpu.trees_fused is True
    sv = gpu.shap_values(X)
    fx = logit(pred(X))
    for o in range(2):
        assert sv[o].shape == (4, D)
        assert np.allclose(sv[o], sv_cpu[o], atol=5e-4, rtol=5e-3), \
            np.abs(sv[o] - sv_cpu[o]).max()
        total = sv[o].sum(axis=1) + gpu.expected_value[o]
        assert np.abs(total - fx[:, o]).max() < 1e-3


def test_engine_fused_trees_deterministic_and_split(e2e):
    pred, bg, X, sv_cpu, gpu = e2e
    a = gpu.shap_values(X)
    b = gpu.shap_values(X)
    p1 = gpu.shap_values(X[:2], instance_offset=0)
    p2 = gpu.shap_values(X[2:], instance_offset=2)
    for o in range(2):
        assert np.array_equal(a[o], b[o])
        assert np.allclose(a[o], np.concatenate([p1[o], p2[o]]), atol=1e-5)


def test_fused_trees_on_sample_slice(e2e):
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


def test_engine_fused_trees_mixed_buckets(e2e):
    pred, _, _, _, _ = e2e
    bg, X = _e2e_data()
    bg[:, 3] = 0.7                 # constant background column ...
    X[1, 3] = 0.7                  # ... that instance 1 matches: 7 varying
    sv_cpu = _engine(pred, bg, "cpu").shap_values(X)
    gpu = _engine(pred, bg, "cuda")
    sv = gpu.shap_values(X)
    assert gpu._gpu.trees_fused is True
    for o in range(2):
        assert sv[o][1, 3] == 0.0
        assert np.allclose(sv[o], sv_cpu[o], atol=5e-4, rtol=5e-3), \
            np.abs(sv[o] - sv_cpu[o]).max()


def test_engine_deep_tree_falls_back_to_module_path(caplog):
    rng = np.random.Generator(np.random.Philox(key=[79, 0]))
    chain = _chain(65, list(range(D)), rng)
    chain["value"] = chain["value"] * 0.5
    pred = TreeEnsemblePredictor(
        [chain, _stump(2, 0.1, -0.4, 0.6)], D, 2, out_col=[1, 0],
        activation="softmax")
    bg, X = _e2e_data()
    sv_cpu = _engine(pred, bg, "cpu").shap_values(X)
    with caplog.at_level(
            logging.INFO, logger="distributedkernelshap_amd.ops.gpu_engine"):
        gpu = _engine(pred, bg, "cuda")
        sv = gpu.shap_values(X)
        gpu.shap_values(X)
    assert gpu._gpu.trees_fused is False
    reasons = [r for r in caplog.records if "fused tree kernel" in r.getMessage()]
    assert len(reasons) == 1 and "65 internal nodes" in reasons[0].getMessage()
    for o in range(2):
        assert np.allclose(sv[o], sv_cpu[o], atol=5e-4, rtol=5e-3), \
            np.abs(sv[o] - sv_cpu[o]).max()


def test_engine_trees_fp64_mode_matches_cpu_oracle(e2e):
    pred, bg, X, sv_cpu, _ = e2e
    gpu = _engine(pred, bg, "cuda", predict_dtype="fp64")
    sv = gpu.shap_values(X)
    for o in range(2):
        assert np.allclose(sv[o], sv_cpu[o], rtol=0.0, atol=1e-8), \
            np.abs(sv[o] - sv_cpu[o]).max()


def test_engine_trees_bf16_raises(e2e):
    pred, bg, _, _, _ = e2e
    with pytest.raises(ValueError, match="fp32"):
        _engine(pred, bg, "cuda", predict_dtype="bf16")
    with pytest.raises(ValueError, match="fp32"):
        _engine(pred, bg, "cuda", predict_dtype="bf16x2")


def test_engine_trees_module_autocast_bf16_raises(e2e):
    # bf16 features would flip split decisions on the module path
    pred, bg, _, _, _ = e2e
    with pytest.raises(ValueError, match="module_autocast"):
        _engine(pred, bg, "cuda", module_autocast="bf16")


def test_engine_leaves_the_predictor_untouched_and_picklable():
    import pickle

    pred = TreeEnsemblePredictor.random(D, 2, trees=6, depth=3, seed=11)
    bg, X = _e2e_data()
    _engine(pred, bg, "cuda").shap_values(X[:1])
    assert pred._module is None
    clone = pickle.loads(pickle.dumps(pred))
    assert np.array_equal(clone(X), pred(X))


def test_kernel_shap_public_api_sklearn_gradient_boosting():
    from sklearn.ensemble import GradientBoostingClassifier

    from distributedkernelshap_amd import KernelShap
    from distributedkernelshap_amd.models import make_adult_like

    data = make_adult_like(n_instances=8, n_background=25)
    train = make_adult_like(n_instances=200, n_background=1, seed=3).X
    y = (train[:, 0] + train[:, 1] * train[:, 2] > np.median(train[:, 0])).astype(int)
    est = GradientBoostingClassifier(
        n_estimators=15, max_depth=3, random_state=0).fit(train, y)
    pred = TreeEnsemblePredictor.from_sklearn(est)
    ks = KernelShap(pred, link="logit", device="cuda")
    ks.fit(data.background, groups=data.groups, group_names=data.group_names)
    assert ks._explainer._engine._gpu.trees_fused is True
    exp = ks.explain(data.X)
    sv = exp.shap_values
    assert len(sv) == 2
    for o in range(2):
        assert sv[o].shape == (8, 12)
        assert np.isfinite(sv[o]).all()
