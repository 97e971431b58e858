"""One-vs-one fused predict (fused_predict_kernelmachine_pairs) on the GPU:
the kernel against an explicit blend fed to the numpy oracle, and the engine
end to end against the CPU oracle, for MulticlassSVCPredictor.

Bounds: the project's fused-predict bound (atol 2e-5, rtol 1e-4) at kernel
level and atol 5e-4, rtol 5e-3 on the shap values. They apply because the
fp32 torch module, which runs the kernel's epilogue arithmetic on the CPU, is
within a quarter of them on the same inputs (asserted in
``test_multiclass_svc_predictor.py``; measured: at most 8.4e-7 absolute, 1.6 %
of the bound, at the clip-saturated case 6 and below 0.2 % elsewhere).
"""
import logging

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from multiclass_svc_cases import ATOL, RTOL, SHAPES, case  # noqa: E402

from distributedkernelshap_amd.models import (  # noqa: E402
    KernelMachinePredictor,
    MulticlassSVCPredictor,
)
from distributedkernelshap_amd.ops import km_pack  # noqa: E402


@pytest.fixture(scope="module")
def ext():
    from distributedkernelshap_amd.ops import load_extension

    return load_extension()


# ----------------------------------------------------------------------- #
# kernel level

def _run_kernel(ext, p, pred=None):
    dev = "cuda"
    pred = p["pred"] if pred is None else pred
    pack = km_pack.pack_machine(pred.kernel_machine_params(), p["col_group"],
                                p["n_groups"], dev)
    vidx = torch.arange(p["n_groups"], device=dev)
    xparts = km_pack.group_parts(pack, torch.from_numpy(p["x"]).to(dev))
    bgparts = km_pack.group_parts(pack, torch.from_numpy(p["bg"]).to(dev))
    xp = km_pack.image(pack, xparts, vidx)
    bgpn = km_pack.image(pack, bgparts, vidx, negate=True)
    base = km_pack.base(pack, bgparts)
    wbg = torch.from_numpy(p["wbg"]).float().to(dev)
    b, s, _ = p["masks"].shape
    ey = torch.full((b, s, pred.n_out), float("nan"), device=dev)
    km_pack.fused_predict(ext, pack, torch.from_numpy(p["masks"]).to(dev), xp,
                          bgpn, base, wbg, ey)
    torch.cuda.synchronize()
    return ey.double().cpu().numpy()


@pytest.mark.parametrize("shape_id", sorted(SHAPES))
def test_pairs_kernel_vs_blend_reference(ext, shape_id):
    p, ref, keep = case(shape_id)
    # on the reference alone: the ovr exclusion leaves at least 90 %
    assert keep.mean() >= 0.9
    ey = _run_kernel(ext, p)
    assert ey.shape == ref.shape
    assert np.isfinite(ey).all()
    err = np.abs(ey - ref)[keep].max()
    print(f"shape {shape_id}: fp32 max abs err vs blend reference = {err:.3e}"
          f" (max |ref| {np.abs(ref).max():.3g}, "
          f"left out {1 - keep.mean():.3%})")
    assert np.allclose(ey[keep], ref[keep], atol=ATOL, rtol=RTOL), err


def test_pairs_kernel_batch_rows_differ():
    # shape 5 is only a batch-stride guard if the instances really differ
    p, ref, _ = case(5)
    assert np.abs(ref[0] - ref[1]).max() > 1e-3
    assert np.abs(ref[1] - ref[2]).max() > 1e-3


def test_pairs_kernel_clip_shape_saturates(ext):
    # shape 6 only guards the clip if most pair probabilities sit on it
    p, ref, _ = case(6)
    pred = p["pred"]
    from multiclass_svc_cases import blend

    f = pred.raw(blend(p).reshape(-1, pred.n_features))
    i, j = np.triu_indices(pred.n_classes, 1)
    rij = pred.pair_probabilities(f)[:, i, j]
    assert ((rij <= 1e-7) | (rij >= 1.0 - 1e-7)).mean() > 0.5
    ey = _run_kernel(ext, p)
    assert np.isfinite(ey).all()
    # a weighted mean (weights sum to 1) of probability vectors
    assert np.abs(ey.sum(axis=-1) - 1.0).max() < 1e-5


def test_new_class_through_old_entry_is_bit_identical(ext):
    # activation "none" with P = 6 <= 8 takes fused_predict_kernelmachine
    p, _, _ = case(7)
    pred = p["pred"]
    assert pred.n_out == 6 and pred.activation == "none"
    plain = KernelMachinePredictor(
        pred.support_vectors, pred.alpha, pred.intercept, kernel=pred.kernel,
        gamma=pred.gamma, activation="none")
    assert np.array_equal(_run_kernel(ext, p), _run_kernel(ext, p, pred=plain))


def test_pairs_kernel_two_launches_identical(ext):
    for shape_id in (2, 4):
        p, _, _ = case(shape_id)
        assert np.array_equal(_run_kernel(ext, p), _run_kernel(ext, p))


def test_pairs_kernel_outside_envelope_raises(ext):
    p, _, _ = case(2)
    seven = MulticlassSVCPredictor.random(9, 7, n_sv=37, seed=1,
                                          activation="coupling")
    with pytest.raises(RuntimeError, match="envelope"):
        _run_kernel(ext, p, pred=seven)


# ----------------------------------------------------------------------- #
# end to end: d = 8 singleton groups, full enumeration (no sampling noise)

D = 8


def _e2e_data():
    rng = np.random.Generator(np.random.Philox(key=[131, 8]))
    return rng.normal(size=(30, D)), rng.normal(size=(4, D))


def _engine(pred, bg, device, link, **kernel_kw):
    from distributedkernelshap_amd.config import KernelConfig
    from distributedkernelshap_amd.core.engine import KernelShapEngine

    return KernelShapEngine(
        pred, bg, link=link, seed=0, device=device,
        kernels=KernelConfig(**kernel_kw) if kernel_kw else None,
    )


_E2E = {}


def _e2e(name):
    """Predictor, link, data and CPU-oracle values, computed once."""
    if name not in _E2E:
        k, act, link = {"coupling": (3, "coupling", "logit"),
                        "ovr": (4, "ovr", "identity")}[name]
        pred = MulticlassSVCPredictor.random(D, k, n_sv=40, seed=0,
                                             activation=act)
        bg, X = _e2e_data()
        sv_cpu = _engine(pred, bg, "cpu", link).shap_values(X)
        _E2E[name] = (pred, link, bg, X, sv_cpu)
    return _E2E[name]


@pytest.mark.parametrize("name", ["coupling", "ovr"])
def test_engine_fused_multiclass_matches_cpu_oracle(name):
    from distributedkernelshap_amd.core.links import identity, logit

    pred, link, bg, X, sv_cpu = _e2e(name)
    gpu = _engine(pred, bg, "cuda", link)
    assert gpu._gpu.km_fused is True
    sv = gpu.shap_values(X)
    fx = (logit if link == "logit" else identity)(pred(X))
    assert len(sv) == pred.n_classes
    for o in range(pred.n_classes):
        assert sv[o].shape == (4, D)
        err = np.abs(sv[o] - sv_cpu[o]).max()
        print(f"{name} output {o}: max abs shap err vs CPU oracle {err:.3e}")
        assert np.allclose(sv[o], sv_cpu[o], atol=5e-4, rtol=5e-3), err
        total = sv[o].sum(axis=1) + gpu.expected_value[o]
        assert np.abs(total - fx[:, o]).max() < 1e-3


@pytest.mark.parametrize("name", ["coupling", "ovr"])
def test_engine_multiclass_fp64_mode_matches_cpu_oracle(name):
    pred, link, bg, X, sv_cpu = _e2e(name)
    gpu = _engine(pred, bg, "cuda", link, predict_dtype="fp64")
    sv = gpu.shap_values(X)
    for o in range(pred.n_classes):
        assert np.allclose(sv[o], sv_cpu[o], rtol=0.0, atol=1e-8), \
            np.abs(sv[o] - sv_cpu[o]).max()


def test_engine_seven_classes_fall_back_to_module_path(caplog):
    pred = MulticlassSVCPredictor.random(D, 7, n_sv=40, seed=3,
                                         activation="coupling")
    bg, X = _e2e_data()
    bg, X = bg[:10], X[:2]
    sv_cpu = _engine(pred, bg, "cpu", "logit").shap_values(X)
    with caplog.at_level(
            logging.INFO, logger="distributedkernelshap_amd.ops.gpu_engine"):
        gpu = _engine(pred, bg, "cuda", "logit")
        sv = gpu.shap_values(X)
        gpu.shap_values(X)
    assert gpu._gpu.km_fused is False
    reasons = [r for r in caplog.records
               if "fused kernel-machine kernel" in r.getMessage()]
    assert len(reasons) == 1
    assert "7 classes" in reasons[0].getMessage()
    for o in range(7):
        assert np.allclose(sv[o], sv_cpu[o], atol=5e-4, rtol=5e-3), \
            np.abs(sv[o] - sv_cpu[o]).max()


def test_kernel_shap_public_api_multiclass_svc_proba():
    from sklearn.svm import SVC

    from distributedkernelshap_amd import KernelShap
    from distributedkernelshap_amd.models import make_adult_like

    data = make_adult_like(n_instances=8, n_background=25)
    train = make_adult_like(n_instances=240, n_background=1, seed=3).X
    score = train[:, 0] + train[:, 1] * train[:, 2]
    y = np.digitize(score, np.quantile(score, [1 / 3, 2 / 3]))
    est = SVC(kernel="rbf", gamma="scale", probability=True,
              random_state=0).fit(train, y)
    pred = MulticlassSVCPredictor.from_sklearn(est, output="proba")
    ks = KernelShap(pred, link="identity", device="cuda")
    ks.fit(data.background, groups=data.groups, group_names=data.group_names)
    assert ks._explainer._engine._gpu.km_fused is True
    exp = ks.explain(data.X)
    sv = exp.shap_values
    assert len(sv) == 3
    fx = pred(data.X)
    for o in range(3):
        assert sv[o].shape == (8, 12)
        assert np.isfinite(sv[o]).all()
        total = sv[o].sum(axis=1) + ks.expected_value[o]
        assert np.abs(total - fx[:, o]).max() < 1e-3
