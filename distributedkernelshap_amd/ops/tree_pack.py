"""Packed tables for the fused tree predict kernels (``fused_predict_trees``
and, for deep trees, ``fused_predict_trees_walk``).

Everything here is numpy on the host plus plain torch on small tensors: the
tables are built once per engine, ``decision_bits`` runs once at fit for the
background and once per call for the instances.

Per-tree layout (matching ``ops/hip/tree_kernels.hip``):

  internal nodes are renumbered 0..I-1 in preorder with the root at 0, I <= 64,
  so one u64 holds all of a tree's split decisions (bit i = "node i goes left")

  feat, thr   (T, Ipad) int64 / f64   split feature and threshold of node i;
                                      pad slots compare against -inf (bit 0)
  child       (C, 2) u8               child[off_t + i][bit]; bit 1 = left.
                                      < 64: internal node; else 64 + leaf index
                                      within the tree.  C is padded to a
                                      multiple of 8 nodes
  meta        (T, 4) int32            child offset, leaf offset, out col, I
  leaves      (L,) or (L, n_out) f32  leaf values in tree order
  grp_off     (T + 1) int32           CSR over each tree's coalition groups
  grp_id      (E) int32               group id
  grp_mask    (E) int64               u64 mask of the tree's nodes that split
                                      on a feature of that group

A tree that is a single leaf gets one dummy internal node whose children are
both that leaf.

Deep trees (``fused_predict_trees_walk``, ``ops/hip/tree_walk_kernels.hip``)
use a second, independent set of tables built by ``pack_trees_walk``:

  nodes       (R, 4) int32            one 16-byte record per node, internal
                                      nodes and leaves alike.  The nodes of a
                                      tree are numbered in preorder and the
                                      trees follow each other, so record
                                      ``roots[t]`` is tree t's root and the
                                      left child of record i is record i + 1.
                                      split: [0] the bits of the float32
                                               ``floor_f32(threshold)``
                                             [1] feature (>= 0)
                                             [2] coalition group of the feature
                                             [3] record index of the right child
                                      leaf:  [0] the bits of the float32 leaf
                                                 value (scalar leaves; the
                                                 kernel reads it here), 0 for
                                                 vector leaves
                                             [1] -1
                                             [2] output column (0 for vector
                                                 leaves)
                                             [3] row of ``leaves``
                                      A float32 row value v goes left when
                                      ``v <= thr32``.
  roots       (T,) int32              record index of each tree's root
  leaves      (L,) or (L, n_out) f32  leaf values, trees in order, a tree's
                                      leaves in preorder (the kernel reads
                                      the vector form only)

Routed ensembles (``RoutedTreeEnsemblePredictor``: ``params`` carries a
``"routing"`` entry) add to both sets of tables:

  missing_left (T, Ipad) bool         bit-register pack only: a missing value
                                      goes left at node i (pad slots: False)
  cat_row     (T, Ipad) int64         bit-register pack only: -1 for a
                                      numeric split, else a row of cat_left
  cat_left    (max(C, 1), 8)          256 bits per categorical split, bit c
                                      set = "category code c goes left";
                                      int64 holding u32 words in the
                                      bit-register pack (torch), int32 bit
                                      patterns in the walk pack (kernel)
  categories  {feature: f32 tensor}   sorted known category values of the
                                      features that ``encode_rows`` replaces
                                      by their category index (NaN when
                                      absent)

and the walk record of a split changes to

  [0] the float32 threshold bits, or the cat_left row of a categorical split
  [2] the coalition group in the low 16 bits, ``WALK_FLAG_MISSING_LEFT`` and
      ``WALK_FLAG_CATEGORICAL`` above them (groups are <= 1,024)

The rule at a node, for the encoded float32 value v: a numeric split sends
NaN by missing_left and otherwise ``v <= thr32`` left; a categorical split
sends NaN, ``v < 0`` and ``v >= 256`` by missing_left and otherwise
``trunc(v)`` left iff its bit is set.
"""
from __future__ import annotations

import numpy as np

MAX_NODES = 64        # internal nodes per tree
MAX_NOUT = 8
MAX_TREES = 1024
LDS_BYTES = 160 * 1024
_THREADS = 1024       # workgroup size of the kernel (reduction scratch)

# envelope of the walk kernel for deep trees
WALK_MAX_DEPTH = 64       # step bound of one walk
WALK_MAX_GROUPS = 1024    # group bitset: 16 u64 words per sample in LDS
WALK_MAX_FEATURES = 4096  # x row: 16 KiB of LDS
WALK_MAX_RECORDS = 2**31 - 1
# routed walk record [2]: flags above the group
WALK_GROUP_MASK = 0xFFFF
WALK_FLAG_MISSING_LEFT = 1 << 30
WALK_FLAG_CATEGORICAL = 1 << 29
CAT_CODES = 256           # category codes a bitset row holds

ACT_CODE = {"none": 0, "sigmoid": 1, "softmax": 2}


def _internal_counts(trees):
    return [max(1, int((np.asarray(tr["left"]) >= 0).sum())) for tr in trees]


def _child_rows(counts) -> int:
    return (sum(counts) + 7) // 8 * 8


def lds_bytes_min(n_trees: int, child_rows: int, n_out: int) -> int:
    """LDS the kernel needs at its narrowest tile (16 samples per workgroup):
    8 B x 16 per tree for the node masks (at least the reduction scratch)
    plus 2 B per internal node for the child table."""
    no = 1 if n_out <= 1 else 2 if n_out <= 2 else 4 if n_out <= 4 else 8
    return max(n_trees * 16 * 8, _THREADS * no * 4) + 2 * child_rows


def envelope_reason(params: dict):
    """None when the ensemble fits the fused kernel, else a one-line reason."""
    trees = params["trees"]
    counts = _internal_counts(trees)
    worst = int(np.argmax(counts))
    if counts[worst] > MAX_NODES:
        return (f"tree {worst} has {counts[worst]} internal nodes "
                f"(supported: <= {MAX_NODES})")
    if params["n_out"] > MAX_NOUT:
        return f"n_out {params['n_out']} (supported: <= {MAX_NOUT})"
    if len(trees) > MAX_TREES:
        return f"{len(trees)} trees (supported: <= {MAX_TREES})"
    need = lds_bytes_min(len(trees), _child_rows(counts), params["n_out"])
    if need > LDS_BYTES:
        return (f"{len(trees)} trees with {sum(counts)} internal nodes need "
                f"{need} B of LDS (supported: <= {LDS_BYTES})")
    return None


def pack_trees(params: dict, col_group, device) -> dict:
    """Device tables for ``tree_params()`` output ``params`` and the
    feature -> group map ``col_group`` (D,). No envelope check: the kernel
    binding is the one place that refuses unsupported ensembles (a tree with
    more than 64 internal nodes is packed with truncated codes and must not
    be walked)."""
    import torch as t

    trees = params["trees"]
    n_out = int(params["n_out"])
    col_group = np.asarray(col_group, dtype=np.int64)
    vector = params["out_col"] is None
    counts = _internal_counts(trees)
    ipad = max(MAX_NODES, max(counts))
    n_trees = len(trees)
    feat = np.zeros((n_trees, ipad), dtype=np.int64)
    thr = np.full((n_trees, ipad), -np.inf)
    routing = params.get("routing")
    if routing is not None:
        # pad slots: not missing-left, numeric, threshold -inf -> bit 0
        mleft = np.zeros((n_trees, ipad), dtype=bool)
        crow = np.full((n_trees, ipad), -1, dtype=np.int64)
    child = np.zeros((_child_rows(counts), 2), dtype=np.int64)
    meta = np.zeros((n_trees, 4), dtype=np.int32)
    leaves, grp_off, grp_id, grp_mask = [], [0], [], []
    coff = loff = 0
    for ti, tr in enumerate(trees):
        left = np.asarray(tr["left"])
        right = np.asarray(tr["right"])
        value = np.asarray(tr["value"], dtype=np.float64)
        internal = left >= 0
        # preorder renumbering of internal nodes and of leaves
        code = np.zeros(left.shape[0], dtype=np.int64)
        n_int = n_leaf = 0
        order, stack = [], [0]
        while stack:
            i = stack.pop()
            if internal[i]:
                code[i] = n_int
                n_int += 1
                order.append(i)
                stack.append(int(right[i]))
                stack.append(int(left[i]))
            else:
                code[i] = MAX_NODES + n_leaf
                n_leaf += 1
                leaves.append(value[i])
        if n_int == 0:
            # single leaf: a dummy split on feature 0 whose sides agree
            child[coff] = MAX_NODES
            n_int = 1
        else:
            for i in order:
                k = code[i]
                feat[ti, k] = tr["feature"][i]
                thr[ti, k] = tr["threshold"][i]
                if routing is not None:
                    mleft[ti, k] = tr["missing_left"][i]
                    crow[ti, k] = tr["cat_row"][i]
                child[coff + k, 1] = code[left[i]]
                child[coff + k, 0] = code[right[i]]
            by_group: dict = {}
            for i in order:
                g = int(col_group[tr["feature"][i]])
                by_group[g] = by_group.get(g, 0) | (1 << int(code[i] % 64))
            for g in sorted(by_group):
                grp_id.append(g)
                grp_mask.append(by_group[g])
        grp_off.append(len(grp_id))
        meta[ti] = (coff, loff, 0 if vector else int(params["out_col"][ti]), n_int)
        coff += n_int
        loff += n_leaf
    leaves = np.asarray(leaves, dtype=np.float32)
    if not grp_id:                       # every tree is a single leaf
        grp_id, grp_mask = [0], [0]
    gm = np.asarray(grp_mask, dtype=np.uint64).view(np.int64)

    def dev(a):
        return t.from_numpy(np.ascontiguousarray(a)).to(device)

    extra = {}
    if routing is not None:
        extra = {"routed": True, "missing_left": dev(mleft), "cat_row": dev(crow),
                 "cat_left": dev(_cat_rows(routing).astype(np.int64)),
                 "categories": _category_tensors(routing, device)}
    return {
        **extra,
        "n_trees": n_trees, "n_out": n_out, "leaf_mode": 1 if vector else 0,
        "max_internal": int(max(counts)),
        "feat": dev(feat), "thr": dev(thr),
        "child": dev(np.minimum(child, 255).astype(np.uint8)),
        "meta": dev(meta), "leaves": dev(leaves),
        "grp_off": dev(np.asarray(grp_off, dtype=np.int32)),
        "grp_id": dev(np.asarray(grp_id, dtype=np.int32)),
        "grp_mask": dev(gm),
        "base": dev(np.asarray(params["base"], dtype=np.float32)),
        "scale": float(params["scale"]),
        "act": ACT_CODE[params["activation"]],
    }


def _cat_rows(routing: dict) -> np.ndarray:
    """(max(C, 1), 8) uint32: the bitset table, never empty, so that a
    clamped row index always names a row."""
    cat_left = np.asarray(routing["cat_left"], dtype=np.uint32).reshape(-1, 8)
    if cat_left.shape[0] == 0:
        cat_left = np.zeros((1, 8), dtype=np.uint32)
    return cat_left


def _category_tensors(routing: dict, device) -> dict:
    import torch as t

    return {int(f): t.from_numpy(np.asarray(c, dtype=np.float32)).to(device)
            for f, c in sorted(routing["categories"].items())}


def encode_rows(pack: dict, rows):
    """float32 rows as the nodes of a routed pack see them: every feature
    with known categories is replaced by the index of its value among them,
    or NaN when it is not there (one ``searchsorted`` per such feature).
    A pack without routing gets the float32 rows themselves."""
    import torch as t

    x = rows.float()
    cats = pack.get("categories")
    if not cats:
        return x.contiguous()
    x = x.clone()
    for f, c in cats.items():
        v = x[:, f].contiguous()
        k = t.searchsorted(c, v).clamp_(max=c.shape[0] - 1)
        x[:, f] = t.where(c[k] == v, k.to(v.dtype), t.full_like(v, float("nan")))
    return x.contiguous()


def decision_bits(pack: dict, rows):
    """(R, T) int64: bit i of [r, t] is ``float64(float32(rows[r, feat_i]))
    <= thr_i`` for internal node i of tree t — sklearn's comparison rule,
    evaluated in torch on the device of ``rows``. A routed pack encodes the
    rows and applies the routing rule of the module docstring instead."""
    import torch as t

    if pack.get("routed"):
        return _decision_bits_routed(pack, rows)
    feat, thr = pack["feat"], pack["thr"]
    n_trees, ipad = feat.shape
    x = rows.float().double()
    shifts = t.arange(ipad, device=x.device, dtype=t.int64) % 64
    out = t.empty(x.shape[0], n_trees, dtype=t.int64, device=x.device)
    step = max(1, (1 << 24) // (n_trees * ipad))
    flat = feat.reshape(-1)
    for lo in range(0, x.shape[0], step):
        xs = x[lo : lo + step]
        go_left = xs[:, flat].view(-1, n_trees, ipad) <= thr[None]
        # disjoint bits: the wrapping int64 sum is the OR, bit 63 included
        out[lo : lo + step] = (go_left.to(t.int64) << shifts).sum(dim=-1)
    return out


def _decision_bits_routed(pack: dict, rows):
    import torch as t

    feat, thr = pack["feat"], pack["thr"]
    mleft, crow, cat_left = pack["missing_left"], pack["cat_row"], pack["cat_left"]
    is_cat = crow >= 0
    any_cat = bool(is_cat.any())
    n_trees, ipad = feat.shape
    x = encode_rows(pack, rows).double()
    shifts = t.arange(ipad, device=x.device, dtype=t.int64) % 64
    out = t.empty(x.shape[0], n_trees, dtype=t.int64, device=x.device)
    step = max(1, (1 << 23) // (n_trees * ipad))
    flat = feat.reshape(-1)
    for lo in range(0, x.shape[0], step):
        v = x[lo : lo + step][:, flat].view(-1, n_trees, ipad)
        nan = v != v
        go_left = t.where(nan, mleft[None], v <= thr[None])
        if any_cat:
            missing = nan | (v < 0) | (v >= CAT_CODES)
            c = t.where(missing, t.zeros_like(v), v).long()      # truncates
            word = cat_left[crow.clamp(min=0)[None].expand_as(c), c >> 5]
            bit = ((word >> (c & 31)) & 1) != 0
            go_left = t.where(is_cat[None],
                              t.where(missing, mleft[None], bit), go_left)
        out[lo : lo + step] = (go_left.to(t.int64) << shifts).sum(dim=-1)
    return out


def _preorder(left, right):
    """Nodes of one tree in preorder (left subtree first) and its depth in
    splits along the longest path."""
    order, depth = [], 0
    stack = [(0, 0)]
    while stack:
        i, d = stack.pop()
        order.append(i)
        if left[i] >= 0:
            stack.append((int(right[i]), d + 1))
            stack.append((int(left[i]), d + 1))
        elif d > depth:
            depth = d
    return order, depth


def walk_envelope_reason(params: dict, n_features: int, n_groups: int):
    """None when the ensemble fits the walk kernel for deep trees, else a
    one-line reason."""
    depth = max(_preorder(np.asarray(tr["left"]), np.asarray(tr["right"]))[1]
                for tr in params["trees"])
    if depth > WALK_MAX_DEPTH:
        return f"depth {depth} (walk kernel: <= {WALK_MAX_DEPTH})"
    if params["n_out"] > MAX_NOUT:
        return f"n_out {params['n_out']} (walk kernel: <= {MAX_NOUT})"
    if n_groups > WALK_MAX_GROUPS:
        return f"{n_groups} groups (walk kernel: <= {WALK_MAX_GROUPS})"
    if n_features > WALK_MAX_FEATURES:
        return f"{n_features} features (walk kernel: <= {WALK_MAX_FEATURES})"
    records = sum(len(tr["left"]) for tr in params["trees"])
    if records > WALK_MAX_RECORDS:
        return f"{records} nodes (walk kernel: <= {WALK_MAX_RECORDS})"
    return None


def pack_trees_walk(params: dict, col_group, device) -> dict:
    """Device tables of the walk kernel (layout in the module docstring) for
    ``tree_params()`` output ``params`` and the feature -> group map
    ``col_group`` (D,). No envelope check: the kernel binding is the one
    place that refuses unsupported ensembles."""
    import torch as t

    from ..models.tree_module import floor_f32

    trees = params["trees"]
    col_group = np.asarray(col_group, dtype=np.int64)
    vector = params["out_col"] is None
    routing = params.get("routing")
    nodes, roots, leaves = [], [], []
    off = n_leaf = max_depth = 0
    for ti, tr in enumerate(trees):
        left = np.asarray(tr["left"], dtype=np.int64)
        right = np.asarray(tr["right"], dtype=np.int64)
        feature = np.asarray(tr["feature"], dtype=np.int64)
        order, depth = _preorder(left, right)
        order = np.asarray(order, dtype=np.int64)
        max_depth = max(max_depth, depth)
        pos = np.empty(left.shape[0], dtype=np.int64)
        pos[order] = np.arange(order.shape[0]) + off
        internal = left[order] >= 0
        feat = np.where(internal, feature[order], 0)
        leaf_row = n_leaf + np.cumsum(~internal) - 1
        rec = np.empty((order.shape[0], 4), dtype=np.int32)
        thr32 = floor_f32(np.asarray(tr["threshold"], dtype=np.float64)[order])
        value = np.asarray(tr["value"], dtype=np.float64)[order]
        leaf_bits = (np.zeros(order.shape[0], dtype=np.int32) if vector
                     else value.astype(np.float32).view(np.int32))
        rec[:, 0] = np.where(internal, thr32.view(np.int32), leaf_bits)
        rec[:, 1] = np.where(internal, feat, -1)
        group = col_group[feat]
        if routing is not None:
            crow = np.asarray(tr["cat_row"], dtype=np.int64)[order]
            cat = internal & (crow >= 0)
            mleft = internal & np.asarray(tr["missing_left"], dtype=bool)[order]
            rec[:, 0] = np.where(cat, crow, rec[:, 0])
            group = (group & WALK_GROUP_MASK) \
                | np.where(mleft, WALK_FLAG_MISSING_LEFT, 0) \
                | np.where(cat, WALK_FLAG_CATEGORICAL, 0)
        rec[:, 2] = np.where(internal, group,
                             0 if vector else int(params["out_col"][ti]))
        rec[:, 3] = np.where(internal, pos[np.maximum(right[order], 0)], leaf_row)
        nodes.append(rec)
        roots.append(off)
        leaves.append(value[~internal])
        off += order.shape[0]
        n_leaf += int((~internal).sum())

    def dev(a):
        return t.from_numpy(np.ascontiguousarray(a)).to(device)

    extra = {}
    if routing is not None:
        extra = {"routed": True,
                 "cat_left": dev(_cat_rows(routing).view(np.int32)),
                 "categories": _category_tensors(routing, device)}
    return {
        **extra,
        "n_trees": len(trees), "n_out": int(params["n_out"]),
        "leaf_mode": 1 if vector else 0, "max_depth": int(max_depth),
        "nodes": dev(np.concatenate(nodes)),
        "roots": dev(np.asarray(roots, dtype=np.int32)),
        "leaves": dev(np.concatenate(leaves).astype(np.float32)),
        "base": dev(np.asarray(params["base"], dtype=np.float32)),
        "scale": float(params["scale"]),
        "act": ACT_CODE[params["activation"]],
    }


def fused_predict_walk(ext, pack: dict, masks, vmap, x, bg, wbg, ey):
    """Launch ``fused_predict_trees_walk`` with the packed tables; ``x``
    (B, D) and ``bg`` (N, D) are the float32 rows themselves, for a routed
    pack the rows that ``encode_rows`` returns."""
    if pack.get("routed"):
        ext.fused_predict_trees_walk(
            masks, vmap, x, bg, pack["nodes"], pack["roots"], pack["leaves"],
            pack["base"], pack["scale"], wbg, ey, pack["act"],
            pack["leaf_mode"], pack["max_depth"], cat_left=pack["cat_left"],
        )
        return ey
    ext.fused_predict_trees_walk(
        masks, vmap, x, bg, pack["nodes"], pack["roots"], pack["leaves"],
        pack["base"], pack["scale"], wbg, ey, pack["act"], pack["leaf_mode"],
        pack["max_depth"],
    )
    return ey


def fused_predict(ext, pack: dict, masks, vmap, dx, dbg, wbg, ey):
    """Launch ``fused_predict_trees`` with the packed tables."""
    ext.fused_predict_trees(
        masks, vmap, dx, dbg, pack["child"], pack["meta"], pack["leaves"],
        pack["grp_off"], pack["grp_id"], pack["grp_mask"], pack["base"],
        pack["scale"], wbg, ey, pack["act"], pack["leaf_mode"],
        pack["max_internal"],
    )
    return ey
