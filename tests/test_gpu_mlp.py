"""Fused MLP predict (fused_predict_mlp) on the GPU: the kernel against an
explicit-blend fp64 reference, the bf16 variant against a bf16 emulation, and
the engine end to end against the CPU oracle."""
import logging

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from distributedkernelshap_amd.models import MLPPredictor  # noqa: E402
from distributedkernelshap_amd.ops import mlp_pack  # noqa: E402


@pytest.fixture(scope="module")
def ext():
    from distributedkernelshap_amd.ops import load_extension

    return load_extension()


# ----------------------------------------------------------------------- #
# kernel level

def _chunked_groups(d, m):
    cuts = np.linspace(0, d, m + 1).round().astype(int)
    return [list(range(cuts[i], cuts[i + 1])) for i in range(m)]


# (D, groups, N, S, hidden, n_out, output act, B) — each the smallest shape
# that breaks one indexing assumption
SHAPES = {
    # N < 16, S not a tile multiple, unequal groups
    1: (7, [[0], [1, 2], [3], [4, 5, 6]], 3, 70, [16], 1, "sigmoid", 1),
    # M % 4 != 0, N crosses a 16 boundary, width changes between layers
    2: (9, _chunked_groups(9, 5), 19, 70, [48, 16], 2, "softmax", 1),
    # hidden 40 needs zero padding to 48, three layers, odd n_out
    3: (9, _chunked_groups(9, 5), 19, 70, [40, 32, 16], 3, "softmax", 1),
    # M crosses 32, maximum width, maximum n_out, S crosses two tiles
    4: (33, [[j] for j in range(33)], 2, 130, [256], 8, "none", 1),
    # B = 3 with distinct x per instance: the batch stride
    5: (9, _chunked_groups(9, 5), 19, 70, [48, 16], 2, "softmax", 3),
}


def _problem(shape_id):
    d, groups, n, s, hidden, n_out, act, b = SHAPES[shape_id]
    rng = np.random.Generator(np.random.Philox(key=[41, shape_id]))
    weights, biases = [], []
    prev = d
    for width in hidden + [n_out]:
        weights.append(rng.normal(0.0, 1.0 / np.sqrt(prev), size=(width, prev)))
        biases.append(rng.normal(0.0, 0.1, size=(width,)))
        prev = width
    x = rng.normal(size=(b, d))
    bg = rng.normal(size=(n, d))
    wbg = rng.uniform(0.2, 1.0, size=n)          # non-uniform
    wbg /= wbg.sum()
    masks = (rng.uniform(size=(b, s, len(groups))) < 0.5).astype(np.uint8)
    col_group = np.empty(d, dtype=np.int64)
    for gi, g in enumerate(groups):
        col_group[g] = gi
    return dict(weights=weights, biases=biases, act=act, x=x, bg=bg, wbg=wbg,
                masks=masks, col_group=col_group, n_groups=len(groups),
                n_out=n_out)


def _blend(p, dtype=torch.float64):
    """(B, S, N, D) perturbation rows — the explicit blend the kernel never
    materialises (CPU torch)."""
    full = torch.from_numpy(p["masks"]).bool()[:, :, p["col_group"]]  # (B,S,D)
    x = torch.from_numpy(p["x"]).to(dtype)
    bg = torch.from_numpy(p["bg"]).to(dtype)
    return torch.where(full[:, :, None, :], x[:, None, None, :],
                       bg[None, None, :, :])


def _out_act(z, act):
    if act == "softmax":
        return torch.softmax(z, dim=-1)
    if act == "sigmoid":
        return torch.sigmoid(z)
    return z


def _reference_f64(p):
    h = _blend(p)
    ws = [torch.from_numpy(w) for w in p["weights"]]
    bs = [torch.from_numpy(b) for b in p["biases"]]
    for w, b in zip(ws[:-1], bs[:-1]):
        h = torch.relu(h @ w.T + b)
    pr = _out_act(h @ ws[-1].T + bs[-1], p["act"])
    return torch.einsum("bsno,n->bso", pr, torch.from_numpy(p["wbg"])).numpy()


def _emulate_bf16(p):
    """Operands and stored activations rounded to bf16, fp32 accumulation,
    final layer / activation / reduction in fp32 (CPU torch)."""
    bf = torch.bfloat16
    h = _blend(p, torch.float32).to(bf).float()
    ws = [torch.from_numpy(w).float() for w in p["weights"]]
    bs = [torch.from_numpy(b).float() for b in p["biases"]]
    for w, b in zip(ws[:-1], bs[:-1]):
        h = torch.relu(h @ w.to(bf).float().T + b).to(bf).float()
    pr = _out_act(h @ ws[-1].T + bs[-1], p["act"])
    wbg = torch.from_numpy(p["wbg"]).float()
    return torch.einsum("bsno,n->bso", pr, wbg).double().numpy()


_REF = {}


def _ref(shape_id):
    """Problem + fp64 reference, computed once and shared (never mutated)."""
    if shape_id not in _REF:
        p = _problem(shape_id)
        _REF[shape_id] = (p, _reference_f64(p))
    return _REF[shape_id]


def _run_kernel(ext, p, dtype, weights=None, biases=None):
    dev = "cuda"
    weights = p["weights"] if weights is None else weights
    biases = p["biases"] if biases is None else biases
    pack = mlp_pack.pack_mlp_weights(weights, biases, dtype, dev)
    colg = torch.from_numpy(p["col_group"]).to(dev)
    g = p["n_groups"]
    vidx = torch.arange(g, device=dev)
    bg64 = torch.from_numpy(p["bg"]).to(dev)
    x64 = torch.from_numpy(p["x"]).to(dev)
    bgp1n = mlp_pack.first_layer_image(
        pack, mlp_pack.group_parts(pack, bg64, colg, g), vidx, negate=True)
    xp1 = mlp_pack.first_layer_image(
        pack, mlp_pack.group_parts(pack, x64, colg, g), vidx)
    base1 = mlp_pack.base1(pack, bg64)
    masks = torch.from_numpy(p["masks"]).to(dev)
    wbg = torch.from_numpy(p["wbg"]).float().to(dev)
    b, s, _ = p["masks"].shape
    ey = torch.full((b, s, weights[-1].shape[0]), float("nan"), device=dev)
    ext.fused_predict_mlp(
        masks, xp1, bgp1n, base1, pack["hidden_w"], pack["hidden_b"],
        pack["wout"], pack["bout"], wbg, ey, mlp_pack.ACT_CODE[p["act"]], 0,
    )
    torch.cuda.synchronize()
    return ey.double().cpu().numpy()


@pytest.mark.parametrize("shape_id", sorted(SHAPES))
def test_fused_mlp_fp32_vs_fp64_reference(ext, shape_id):
    p, ref = _ref(shape_id)
    ey = _run_kernel(ext, p, torch.float32)
    assert ey.shape == ref.shape
    err = np.abs(ey - ref).max()
    print(f"shape {shape_id}: fp32 max abs err vs fp64 = {err:.3e}")
    assert np.allclose(ey, ref, atol=2e-5, rtol=1e-4), err


def test_fused_mlp_batch_rows_differ(ext):
    # shape 5 is only a batch-stride guard if the instances really differ
    p, ref = _ref(5)
    assert np.abs(ref[0] - ref[1]).max() > 1e-3
    assert np.abs(ref[1] - ref[2]).max() > 1e-3


def _widened(p, hidden):
    """The problem's data with a fresh network of the given hidden widths."""
    rng = np.random.Generator(np.random.Philox(key=[43, len(hidden)]))
    weights, biases = [], []
    prev = p["x"].shape[1]
    for width in hidden + [p["n_out"]]:
        weights.append(rng.normal(0.0, 0.1, size=(width, prev)))
        biases.append(np.zeros(width))
        prev = width
    return weights, biases


def test_fused_mlp_width_outside_envelope_raises(ext):
    p, _ = _ref(1)
    weights, biases = _widened(p, [272])
    with pytest.raises(RuntimeError, match="envelope"):
        _run_kernel(ext, p, torch.float32, weights, biases)


def test_fused_mlp_four_hidden_layers_raises(ext):
    p, _ = _ref(1)
    weights, biases = _widened(p, [16, 16, 16, 16])
    with pytest.raises(RuntimeError, match="envelope"):
        _run_kernel(ext, p, torch.float32, weights, biases)


@pytest.mark.parametrize("shape_id", [2, 4])
def test_fused_mlp_bf16_vs_emulation(ext, shape_id):
    """bf16 variant: error against fp64 within 2x the error of a torch bf16
    emulation (a different accumulation order flips bf16 roundings of
    individual activations — an effect of the same order as the error)."""
    p, ref = _ref(shape_id)
    ey = _run_kernel(ext, p, torch.bfloat16)
    kernel_err = np.abs(ey - ref).max()
    emu_err = np.abs(_emulate_bf16(p) - ref).max()
    print(f"shape {shape_id}: bf16 kernel err {kernel_err:.3e}, "
          f"emulation err {emu_err:.3e}")
    assert np.isfinite(ey).all()
    assert kernel_err <= 2.0 * emu_err, (
        f"bf16 kernel max abs err {kernel_err:.3e} vs fp64 exceeds 2x the "
        f"bf16 emulation's {emu_err:.3e}"
    )


# ----------------------------------------------------------------------- #
# end to end: d = 8 singleton groups, full enumeration (no sampling noise)

D = 8


def _e2e_data():
    rng = np.random.Generator(np.random.Philox(key=[47, 8]))
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
    """Predictor, data, CPU-oracle values and one fused fp32 GPU engine."""
    pred = MLPPredictor.random(D, 2, hidden=32, layers=2)
    bg, X = _e2e_data()
    sv_cpu = _engine(pred, bg, "cpu").shap_values(X)
    return pred, bg, X, sv_cpu, _engine(pred, bg, "cuda")


def test_engine_fused_mlp_matches_cpu_oracle(e2e):
    from distributedkernelshap_amd.core.links import logit

    pred, bg, X, sv_cpu, gpu = e2e
    assert gpu._gpu.mlp_fused is True
    sv = gpu.shap_values(X)
    fx = logit(pred(X))
    for o in range(2):
        assert sv[o].shape == (4, D)
        assert np.allclose(sv[o], sv_cpu[o], atol=5e-4, rtol=5e-3), \
            np.abs(sv[o] - sv_cpu[o]).max()
        total = sv[o].sum(axis=1) + gpu.expected_value[o]
        assert np.abs(total - fx[:, o]).max() < 1e-3


def test_engine_fused_mlp_deterministic_and_split(e2e):
    pred, bg, X, sv_cpu, gpu = e2e
    a = gpu.shap_values(X)
    b = gpu.shap_values(X)
    p1 = gpu.shap_values(X[:2], instance_offset=0)
    p2 = gpu.shap_values(X[2:], instance_offset=2)
    for o in range(2):
        assert np.array_equal(a[o], b[o])
        assert np.allclose(a[o], np.concatenate([p1[o], p2[o]]), atol=1e-5)


def test_fused_mlp_on_sample_slice(e2e):
    """The sample-sharded path hands the shared non-linear helper a slice of
    the sample axis: the slice's ey equals the same rows of the full call
    (per-row arithmetic does not depend on the row's tile position; fp32
    rounding-level bound)."""
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


def test_engine_fused_mlp_mixed_buckets(e2e):
    pred, _, _, _, _ = e2e
    bg, X = _e2e_data()
    bg[:, 3] = 0.7                 # constant background column ...
    X[1, 3] = 0.7                  # ... that instance 1 matches: 7 varying
    sv_cpu = _engine(pred, bg, "cpu").shap_values(X)
    gpu = _engine(pred, bg, "cuda")
    sv = gpu.shap_values(X)
    assert gpu._gpu.mlp_fused is True
    for o in range(2):
        assert sv[o][1, 3] == 0.0
        assert np.allclose(sv[o], sv_cpu[o], atol=5e-4, rtol=5e-3), \
            np.abs(sv[o] - sv_cpu[o]).max()


def test_engine_mlp_tanh_falls_back_to_module_path(caplog):
    pred = MLPPredictor.random(D, 2, hidden=32, layers=2,
                               hidden_activation="tanh")
    bg, X = _e2e_data()
    sv_cpu = _engine(pred, bg, "cpu").shap_values(X)
    with caplog.at_level(
            logging.INFO, logger="distributedkernelshap_amd.ops.gpu_engine"):
        gpu = _engine(pred, bg, "cuda")
        sv = gpu.shap_values(X)
        gpu.shap_values(X)
    assert gpu._gpu.mlp_fused is False
    reasons = [r for r in caplog.records if "fused MLP kernel" in r.getMessage()]
    assert len(reasons) == 1 and "tanh" in reasons[0].getMessage()
    for o in range(2):
        assert np.allclose(sv[o], sv_cpu[o], atol=5e-4, rtol=5e-3), \
            np.abs(sv[o] - sv_cpu[o]).max()


def test_engine_mlp_fp64_mode_matches_cpu_oracle(e2e):
    pred, bg, X, sv_cpu, _ = e2e
    gpu = _engine(pred, bg, "cuda", predict_dtype="fp64")
    sv = gpu.shap_values(X)
    for o in range(2):
        assert np.allclose(sv[o], sv_cpu[o], rtol=0.0, atol=1e-8), \
            np.abs(sv[o] - sv_cpu[o]).max()


def test_engine_mlp_bf16x2_raises(e2e):
    pred, bg, _, _, _ = e2e
    with pytest.raises(ValueError, match="fp32"):
        _engine(pred, bg, "cuda", predict_dtype="bf16x2")


def test_engine_mlp_bf16_runs_fused(e2e):
    from distributedkernelshap_amd.core.links import logit

    pred, bg, X, sv_cpu, _ = e2e
    gpu = _engine(pred, bg, "cuda", predict_dtype="bf16")
    assert gpu._gpu.mlp_fused is True
    sv = gpu.shap_values(X)
    fx = logit(pred(X))
    for o in range(2):
        # the totals come from the fp64 forward: local accuracy is exact up
        # to the constrained fp32 solve whatever the predict dtype
        total = sv[o].sum(axis=1) + gpu.expected_value[o]
        assert np.abs(total - fx[:, o]).max() < 1e-3


def test_kernel_shap_public_api_grouped_adult_like():
    from distributedkernelshap_amd import KernelShap
    from distributedkernelshap_amd.models import make_adult_like

    data = make_adult_like(n_instances=8, n_background=25)
    pred = MLPPredictor.random(data.X.shape[1], 2, hidden=32, layers=2, seed=5)
    ks = KernelShap(pred, link="logit", device="cuda")
    ks.fit(data.background, groups=data.groups, group_names=data.group_names)
    assert ks._explainer._engine._gpu.mlp_fused is True
    exp = ks.explain(data.X)
    sv = exp.shap_values
    assert len(sv) == 2
    for o in range(2):
        assert sv[o].shape == (8, 12)
        assert np.isfinite(sv[o]).all()
