"""The user-visible path of the wide linear predict: multi-class linear
predictors (3 and 5..16 outputs) through KernelShapEngine on the GPU. Which
methods ran is recorded by wrapping them, as ``_softmax4_engine`` of
test_gpu_linear_predict_u8.py does.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

_WRAPPED = ("_ey_fused_wide", "_ey_linear_torch", "_ey_fused_linear",
            "_solve_gram", "_solve_torch")

# sum_g phi == link(f(x)) - link(fnull): the bound of
# tests/test_gpu_kernels.py::test_engine_gpu_local_accuracy_adult,
#     assert np.abs(total - fx[:, o]).max() < 1e-3
ADDITIVITY_TOL = 1e-3


class _CountingExt:
    """The extension module with ``wls_solve`` calls counted."""

    def __init__(self, ext, calls):
        self._ext, self._calls = ext, calls

    def __getattr__(self, name):
        fn = getattr(self._ext, name)
        if name != "wls_solve":
            return fn

        def counted(*a, **k):
            self._calls["wls_solve"] = self._calls.get("wls_solve", 0) + 1
            return fn(*a, **k)
        return counted


def _engine(n_out, n_groups, n_bg, link="identity", dtype="fp32"):
    from distributedkernelshap_amd.config import KernelConfig
    from distributedkernelshap_amd.core.engine import KernelShapEngine
    from distributedkernelshap_amd.models import LinearPredictor, make_tabular

    data = make_tabular(n_features=n_groups, n_instances=3,
                        n_background=n_bg, seed=11)
    pred = LinearPredictor.random(n_groups, n_out, seed=11,
                                  activation="softmax")
    eng = KernelShapEngine(
        pred, data.background, groups=data.groups, link=link, seed=0,
        device="cuda", kernels=KernelConfig(predict_dtype=dtype),
    )
    calls = {}
    for meth in _WRAPPED:
        def wrapped(*a, _orig=getattr(eng._gpu, meth), _meth=meth, **k):
            calls[_meth] = calls.get(_meth, 0) + 1
            return _orig(*a, **k)
        setattr(eng._gpu, meth, wrapped)
    eng._gpu.ext = _CountingExt(eng._gpu.ext, calls)
    return eng, data, pred, calls


def _link(name, p):
    from distributedkernelshap_amd.core.links import logit

    return p if name == "identity" else logit(p)


def _run_pair(n_out, n_groups, n_bg, link):
    """fp32 and fp64 engines on the same problem: (r32, r64, calls32, err,
    additivity error of r32)."""
    e32, data, pred, calls = _engine(n_out, n_groups, n_bg, link, "fp32")
    e64, _, _, _ = _engine(n_out, n_groups, n_bg, link, "fp64")
    r32 = e32.shap_values(data.X, nsamples=600, l1_reg=False)
    calls = dict(calls)
    r64 = e64.shap_values(data.X, nsamples=600, l1_reg=False)
    assert len(r32) == n_out and all(r.shape == (3, n_groups) for r in r32)
    assert sum(np.abs(r).sum() for r in r64) > 0
    err = max(np.abs(r32[o] - r64[o]).max() for o in range(n_out))
    fx = _link(link, pred(data.X))
    add = max(
        np.abs(r32[o].sum(axis=1) + e32.expected_value[o] - fx[:, o]).max()
        for o in range(n_out))
    return r32, r64, calls, err, add


def test_engine_softmax10_12_groups_fp32_vs_fp64():
    """10-class softmax, 12 groups, 100 background rows, identity link: the
    bucket runs fused_predict_linear_wide (width 12) and the kernel WLS twice
    (outputs 0..7 and 8..9)."""
    _, _, calls, err, add = _run_pair(10, 12, 100, "identity")
    print(f"engine softmax-10 m=12 fp32 vs fp64: max|dphi|={err:.3e} "
          f"bound=1e-3; additivity {add:.3e} bound={ADDITIVITY_TOL:.0e}; "
          f"calls={calls}")
    assert calls.get("_ey_fused_wide") == 1, calls
    assert "_ey_linear_torch" not in calls and "_ey_fused_linear" not in calls
    assert calls.get("wls_solve") == 2, calls
    assert "_solve_torch" not in calls and "_solve_gram" not in calls
    assert err < 1e-3
    assert add < ADDITIVITY_TOL


def test_engine_softmax3_40_groups_fp32_vs_fp64():
    """3-class softmax, 40 groups: width 4 with one pad class, Mpad 40, and
    a single output chunk on the Gram solve (40 groups are past the kernel
    WLS)."""
    _, _, calls, err, add = _run_pair(3, 40, 100, "identity")
    print(f"engine softmax-3 m=40 fp32 vs fp64: max|dphi|={err:.3e} "
          f"bound=1e-3; additivity {add:.3e} bound={ADDITIVITY_TOL:.0e}; "
          f"calls={calls}")
    assert calls.get("_ey_fused_wide") == 1, calls
    assert "_ey_linear_torch" not in calls and "_ey_fused_linear" not in calls
    assert calls.get("_solve_gram") == 1 and "wls_solve" not in calls, calls
    assert err < 1e-3
    assert add < ADDITIVITY_TOL


def test_engine_softmax10_40_groups_two_gram_chunks_fp32_vs_fp64():
    """10-class softmax, 40 groups: past the kernel WLS, so the two output
    chunks each run the MFMA Gram build + fp64 solve and are concatenated."""
    _, _, calls, err, add = _run_pair(10, 40, 100, "identity")
    print(f"engine softmax-10 m=40 fp32 vs fp64: max|dphi|={err:.3e} "
          f"bound=1e-3; additivity {add:.3e} bound={ADDITIVITY_TOL:.0e}; "
          f"calls={calls}")
    assert calls.get("_ey_fused_wide") == 1, calls
    assert "_ey_linear_torch" not in calls and "_ey_fused_linear" not in calls
    assert calls.get("_solve_gram") == 2, calls
    assert "wls_solve" not in calls and "_solve_torch" not in calls, calls
    assert err < 1e-3
    assert add < ADDITIVITY_TOL


# fp32 against fp64 on identical masks under the logit link, 16 classes, 300
# background rows, 12 groups, nsamples 600: measured once on an MI355X
LOGIT16_MEASURED = 2.709e-06
LOGIT16_BOUND = 4 * LOGIT16_MEASURED


def test_engine_softmax16_300_rows_logit_fp32_vs_fp64():
    """16-class softmax, 300 background rows (Npad 304, beyond the one-tile
    kernels), logit link. The 1e-3 bound of the identity-link tests does not
    carry over: measured max|phi32 - phi64| on an MI355X = 2.709e-06
    (LOGIT16_MEASURED), asserted with a 4x margin, 1.084e-05, for
    instance-to-instance variation."""
    _, _, calls, err, add = _run_pair(16, 12, 300, "logit")
    print(f"engine softmax-16 m=12 N=300 logit fp32 vs fp64: "
          f"max|dphi|={err:.3e} bound={LOGIT16_BOUND:.3e}; additivity {add:.3e} "
          f"bound={ADDITIVITY_TOL:.0e}; calls={calls}")
    assert calls.get("_ey_fused_wide") == 1, calls
    assert "_ey_linear_torch" not in calls and "_ey_fused_linear" not in calls
    assert calls.get("wls_solve") == 2, calls
    assert err < LOGIT16_BOUND
    assert add < ADDITIVITY_TOL


def test_engine_wide_solve_chunk_matches_an_8_output_solve():
    """10 classes: phi[..., :8] of the chunked solve is bit-identical to the
    kernel route handed only the first 8 columns of the same ey_adj and
    total."""
    eng, data, _, calls = _engine(10, 12, 100)
    gpu = eng._gpu
    seen = {}
    orig = gpu._solve_bucket

    def recording(plan, masks, packed, kw, ey_adj, total, l1_reg):
        seen["args"] = (plan, masks.clone(), packed.clone(), kw.clone(),
                        ey_adj.clone(), total.clone(), l1_reg)
        phi = orig(plan, masks, packed, kw, ey_adj, total, l1_reg)
        seen["phi"] = phi.clone()
        return phi

    gpu._solve_bucket = recording
    eng.shap_values(data.X, nsamples=600, l1_reg=False)
    assert seen["phi"].shape == (3, 12, 10)
    assert calls.get("wls_solve") == 2, calls
    plan, masks, packed, kw, ey_adj, total, l1_reg = seen["args"]
    from distributedkernelshap_amd.ops import routes

    assert routes.wls_route(eng.kernels, 12, 8) == "kernel"
    phi8 = orig(plan, masks, packed, kw, ey_adj[..., :8].contiguous(),
                total[:, :8].contiguous(), l1_reg)
    assert calls.get("wls_solve") == 3, calls
    assert phi8.shape == (3, 12, 8)
    assert torch.equal(seen["phi"][..., :8], phi8)


@pytest.mark.parametrize("n_out", [2, 4])
def test_engine_2_and_4_outputs_keep_the_one_tile_kernel(n_out):
    """20 groups: (m-1)+n_out > 16 keeps the bucket off the packed pipeline,
    so the eager loop's predict route is what runs."""
    eng, data, _, calls = _engine(n_out, 20, 100)
    r = eng.shap_values(data.X, nsamples=600, l1_reg=False)
    assert len(r) == n_out
    assert calls.get("_ey_fused_linear") == 1, calls
    assert "_ey_fused_wide" not in calls
