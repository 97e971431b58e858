"""Node table of the walk kernel for deep trees (``pack_trees_walk``) and its
envelope, on the CPU: the records are decoded in numpy from the layout the
module docstring of ``ops/tree_pack.py`` documents."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from distributedkernelshap_amd.models import TreeEnsemblePredictor  # noqa: E402
from distributedkernelshap_amd.ops import tree_pack  # noqa: E402

A32 = np.float32(0.3)
B32 = np.nextafter(A32, np.float32(np.inf))
# float64 thresholds strictly between two neighbouring float32 values: the
# nearest float32 of the first is B32, of the second A32
THR_HI = float(A32) + 0.75 * (float(B32) - float(A32))
THR_LO = float(A32) + 0.25 * (float(B32) - float(A32))


def _stump(feature, thr, lo, hi):
    return {"feature": [feature, -2, -2], "threshold": [thr, 0.0, 0.0],
            "left": [1, -1, -1], "right": [2, -1, -1], "value": [0.0, lo, hi]}


def _single_leaf(v):
    return {"feature": [-2], "threshold": [0.0], "left": [-1], "right": [-1],
            "value": [v]}


def _chain(n_internal, d, rng):
    """The right child of every split is the next split, the left a leaf."""
    n_nodes = 2 * n_internal + 1
    feat = np.full(n_nodes, -2)
    left = np.full(n_nodes, -1)
    right = np.full(n_nodes, -1)
    for i in range(n_internal):
        feat[2 * i] = i % d
        left[2 * i] = 2 * i + 1
        right[2 * i] = 2 * i + 2
    return {"feature": feat, "threshold": rng.normal(-1.0, 0.7, size=n_nodes),
            "left": left, "right": right,
            "value": rng.normal(size=n_nodes)}


def _indexed(pred):
    """The same trees with distinct integers as leaf values (every node of
    every tree its own), so that a value names the leaf that was reached."""
    trees, off = [], 0
    for tr in pred.trees:
        n = len(tr["left"])
        ids = np.arange(off, off + n, dtype=np.float64)
        if pred.vector_leaves:
            ids = ids[:, None] * pred.n_out + np.arange(pred.n_out)[None, :]
        trees.append(dict(tr, value=ids))
        off += n
    return TreeEnsemblePredictor(trees, pred.n_features, pred.n_out,
                                 out_col=pred.out_col)


def _decode_walk(pack, X):
    """Walk the packed records in numpy: (rows, T, n_out) leaf values, zero in
    the columns a scalar leaf does not add to. Checks the step bound."""
    nodes = pack["nodes"].numpy()
    roots = pack["roots"].numpy()
    leaves = pack["leaves"].numpy()
    thr32 = np.ascontiguousarray(nodes[:, 0]).view(np.float32)
    x32 = np.asarray(X).astype(np.float32)
    out = np.zeros((x32.shape[0], roots.shape[0], pack["n_out"]))
    for r in range(x32.shape[0]):
        for t, node in enumerate(roots):
            steps = 0
            while nodes[node, 1] >= 0:
                go_left = x32[r, nodes[node, 1]] <= thr32[node]
                node = node + 1 if go_left else nodes[node, 3]
                steps += 1
            assert steps <= pack["max_depth"] <= tree_pack.WALK_MAX_DEPTH
            assert nodes[node, 1] == -1
            if pack["leaf_mode"] == 1:
                assert nodes[node, 0] == 0
                out[r, t] = leaves[nodes[node, 3]]
            else:
                # a scalar leaf carries its value, equal to its table row
                value = nodes[node, 0:1].view(np.float32)[0]
                assert value == leaves[nodes[node, 3]]
                out[r, t, nodes[node, 2]] = value
    return out


def _oracle_per_tree(pred, X):
    """(rows, T, n_out): what ``TreeEnsemblePredictor.raw`` reaches in each
    tree on its own."""
    cols = []
    for ti, tr in enumerate(pred.trees):
        one = TreeEnsemblePredictor(
            [tr], pred.n_features, pred.n_out,
            out_col=None if pred.vector_leaves else [pred.out_col[ti]])
        cols.append(one.raw(X))
    return np.stack(cols, axis=1)


def _ensembles():
    rng = np.random.Generator(np.random.Philox(key=[83, 0]))
    deep = TreeEnsemblePredictor.random(9, 3, trees=7, depth=9, p_stop=0.05,
                                        seed=5)
    forest = TreeEnsemblePredictor.random(9, 3, trees=4, depth=7, seed=6,
                                          vector_leaves=True)
    mixed = TreeEnsemblePredictor(
        [_single_leaf(0.25), _stump(4, 0.1, -1.0, 1.0), _chain(11, 9, rng),
         _single_leaf(-2.0)], 9, 3, out_col=[2, 0, 1, 1])
    return {"deep": deep, "forest": forest, "mixed": mixed}


@pytest.mark.parametrize("name", ["deep", "forest", "mixed"])
def test_walk_pack_layout_reaches_the_oracles_leaves(name):
    pred = _indexed(_ensembles()[name])
    rng = np.random.Generator(np.random.Philox(key=[83, 1]))
    X = rng.normal(size=(200, 9))
    col_group = np.array([0, 0, 1, 2, 2, 2, 3, 4, 4])
    pack = tree_pack.pack_trees_walk(pred.tree_params(), col_group, "cpu")
    nodes = pack["nodes"].numpy()
    assert nodes.dtype == np.int32 and nodes.shape[1] == 4
    assert nodes.shape[0] == sum(len(tr["left"]) for tr in pred.trees)
    assert pack["roots"].dtype == torch.int32
    assert pack["leaves"].dtype == torch.float32
    assert pack["leaf_mode"] == (1 if pred.vector_leaves else 0)
    # every split carries the coalition group of its feature
    split = nodes[:, 1] >= 0
    assert np.array_equal(nodes[split, 2], col_group[nodes[split, 1]])
    got = _decode_walk(pack, X)
    want = _oracle_per_tree(pred, X)
    assert np.array_equal(got, want)
    # distinct leaf ids: equal values mean the very same leaves
    assert len(np.unique(pack["leaves"].numpy())) == pack["leaves"].numel()


def test_walk_pack_depth_and_counts():
    ens = _ensembles()
    pack = tree_pack.pack_trees_walk(ens["mixed"].tree_params(),
                                     np.zeros(9, dtype=np.int64), "cpu")
    assert pack["max_depth"] == 11
    assert pack["n_trees"] == 4 and pack["roots"].tolist() == [0, 1, 4, 27]
    assert pack["leaves"].numel() == 1 + 2 + 12 + 1


def test_walk_pack_off_grid_thresholds_do_not_flip():
    """A float64 threshold between two float32 neighbours: rows equal to
    either neighbour land on the float64 rule's side. A plain float32 cast
    of THR_HI gives B32 and would send a row equal to B32 left."""
    assert np.float32(THR_HI) == B32 and np.float32(THR_LO) == A32
    pred = TreeEnsemblePredictor(
        [_stump(0, THR_HI, 1.0, 2.0), _stump(0, THR_LO, 3.0, 4.0)], 1, 1)
    pack = tree_pack.pack_trees_walk(pred.tree_params(), [0], "cpu")
    X = np.array([[A32], [B32]], dtype=np.float64)
    got = _decode_walk(pack, X)[:, :, 0]
    assert np.array_equal(got, [[1.0, 3.0], [2.0, 4.0]])
    assert np.array_equal(got.sum(axis=1), pred.raw(X)[:, 0])


def test_walk_envelope_accepts_deep_trees():
    rng = np.random.Generator(np.random.Philox(key=[83, 2]))
    chain = TreeEnsemblePredictor([_chain(64, 9, rng)], 9, 2, out_col=[1])
    assert tree_pack.walk_envelope_reason(chain.tree_params(), 9, 9) is None
    bushy = TreeEnsemblePredictor.random(9, 3, trees=1, depth=9, p_stop=0.0)
    params = bushy.tree_params()
    assert tree_pack._internal_counts(params["trees"])[0] == 511
    assert "511 internal nodes" in tree_pack.envelope_reason(params)
    assert tree_pack.walk_envelope_reason(params, 9, 5) is None


def test_walk_envelope_names_the_cause():
    rng = np.random.Generator(np.random.Philox(key=[83, 3]))
    chain = TreeEnsemblePredictor(
        [_stump(0, 0.0, 1.0, 2.0), _chain(65, 9, rng)], 9, 2, out_col=[0, 1])
    assert "depth 65" in tree_pack.walk_envelope_reason(
        chain.tree_params(), 9, 9)
    wide = TreeEnsemblePredictor([_stump(0, 0.0, 1.0, 2.0)], 9, 9)
    assert "n_out 9" in tree_pack.walk_envelope_reason(wide.tree_params(), 9, 9)
    ok = TreeEnsemblePredictor([_stump(0, 0.0, 1.0, 2.0)], 9, 2).tree_params()
    assert tree_pack.walk_envelope_reason(ok, 4096, 1024) is None
    assert "1025 groups" in tree_pack.walk_envelope_reason(ok, 4096, 1025)
    assert "4097 features" in tree_pack.walk_envelope_reason(ok, 4097, 1024)
