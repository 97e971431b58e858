"""varying_probe (K1p): the varying-pattern probe as two HIP launches, against
the torch chain it replaces (``_varying_matrix_dev`` followed by the
shift-sum), and the engine paths that consume it. All results are integers, so
every kernel comparison is ``torch.equal``."""
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module")
def ext():
    from distributedkernelshap_amd.ops import load_extension

    return load_extension()


# ----------------------------------------------------------------------- #
# inputs

def _col_group(d, g, rng):
    """Every group populated, widths uneven when d > g, columns shuffled."""
    cg = np.concatenate([np.arange(g), rng.integers(0, g, size=d - g)])
    rng.shuffle(cg)
    return cg.astype(np.int64)


def _problem(b, d, g, seed, constant=True):
    """Background with constant columns (whole groups: every even group and
    the last one, so the top bit is in play) and instances whose entries in
    those columns are drawn from the boundary values of the closeness test.
    ``constant=False``: no constant column, every group varies."""
    rng = np.random.Generator(np.random.Philox(key=[seed, 41]))
    cg = _col_group(d, g, rng)
    n = 5
    bg = rng.normal(size=(n, d)).astype(np.float32)
    X = rng.normal(size=(b, d)).astype(np.float32)
    const_cols = np.zeros(d, dtype=bool)
    if constant:
        const_groups = np.zeros(g, dtype=bool)
        const_groups[::2] = True
        const_groups[g - 1] = True
        const_cols = const_groups[cg]
        # |c| in [0.5, 2] or exactly 0 (about a third of the constant columns)
        c = (rng.uniform(0.5, 2.0, size=d) * rng.choice([-1.0, 1.0], size=d))
        c[rng.random(d) < 0.33] = 0.0
        c = c.astype(np.float32)
        bg[:, const_cols] = c[None, const_cols]
        # a seeded random subset of the constant columns, per instance; the
        # rest keep their random value (not close)
        take = (rng.random((b, d)) < 0.93) & const_cols[None]
        kind = rng.choice(4, size=(b, d), p=[0.45, 0.4, 0.1, 0.05])
        one = np.float32(1.0)
        nz = [c,                                   # x == c
              c * (one + np.float32(0.5e-5)),      # close
              c * (one + np.float32(2e-5)),        # not close
              np.full(d, NAN, dtype=np.float32)]   # NaN: varying
        z = [np.zeros(d, dtype=np.float32),
             np.full(d, 0.5e-8, dtype=np.float32),  # c = 0: close
             np.full(d, 2e-8, dtype=np.float32),    # c = 0: not close
             np.full(d, NAN, dtype=np.float32)]
        for k in range(4):
            vals = np.where(c == 0.0, z[k], nz[k])
            sel = take & (kind == k)
            X = np.where(sel, vals[None], X)
    else:
        assert bool((bg.min(axis=0) != bg.max(axis=0)).all())
    return SimpleNamespace(
        X=torch.tensor(X, device=DEV), cg=cg, const_cols=const_cols,
        **_operands(bg, cg, g))


def _operands(bg, cg, g):
    bg_t = torch.tensor(bg, device=DEV)
    bg_min = bg_t.min(dim=0).values
    bg_max = bg_t.max(dim=0).values
    return dict(
        bg_min=bg_min, bg_max=bg_max,
        tol_min=(1e-5 * bg_min.abs() + 1e-8).contiguous(),
        tol_max=(1e-5 * bg_max.abs() + 1e-8).contiguous(),
        col_group=torch.tensor(cg, dtype=torch.int64, device=DEV),
        n_groups=g,
    )


def _reference(p, X):
    """The torch chain: ``_varying_matrix_dev`` then the shift-sum."""
    from distributedkernelshap_amd.ops.gpu_engine import GpuKernelShap

    holder = SimpleNamespace(
        torch=torch, device=torch.device(DEV), bg_min=p.bg_min,
        bg_max=p.bg_max, col_group=p.col_group, n_groups=p.n_groups)
    gbool = GpuKernelShap._varying_matrix_dev(holder, X)
    keys = (gbool.long() << torch.arange(p.n_groups, device=DEV)).sum(dim=1)
    probe = torch.stack([(keys == keys[0]).all().long(), keys[0]])
    return gbool, keys, probe


def _run(ext, p, X, keys=None, probe=None):
    b = X.shape[0]
    if keys is None:
        keys = torch.full((b,), -1, dtype=torch.int64, device=DEV)
        probe = torch.full((2,), -1, dtype=torch.int64, device=DEV)
    ext.varying_probe(X, p.bg_min, p.bg_max, p.tol_min, p.tol_max,
                      p.col_group, p.n_groups, keys, probe)
    return keys, probe


SHAPES = [(1, 50, 12), (3, 7, 7), (257, 50, 12), (1000, 130, 62)]


# ----------------------------------------------------------------------- #
# kernel vs torch

@pytest.mark.parametrize("b,d,g", SHAPES)
def test_varying_probe_equals_torch_chain(ext, b, d, g):
    p = _problem(b, d, g, seed=b + d)
    gbool, kref, pref = _reference(p, p.X)
    keys, probe = _run(ext, p, p.X)
    assert torch.equal(keys, kref)
    assert torch.equal(probe, pref)
    if d == g:
        assert sorted(p.cg.tolist()) == list(range(g))   # one column each
    if b >= 257:
        # both outcomes occur among the constant groups, bit g-1 included,
        # and a group with a non-constant column always varies
        cgroups = np.unique(p.cg[p.const_cols])
        sub = gbool[:, torch.tensor(cgroups, device=DEV)]
        assert bool(sub.any()) and bool((~sub).any())
        top = gbool[:, g - 1]
        assert bool(top.any()) and bool((~top).any())
        vgroups = np.unique(p.cg[~p.const_cols])
        assert bool(gbool[:, torch.tensor(vgroups, device=DEV)].all())
        assert int(pref[0]) == 0


def test_varying_probe_boundary_values(ext):
    """One column per group, one boundary value per group: the expected
    pattern is known without running the torch chain."""
    c = np.array([1.5, 1.5, 1.5, 0.0, 0.0, 0.0, 1.5, 1.5], dtype=np.float32)
    one = np.float32(1.0)
    x = np.array([
        c[0], c[1] * (one + np.float32(0.5e-5)), c[2] * (one + np.float32(2e-5)),
        0.0, 0.5e-8, 2e-8, NAN, 9.0], dtype=np.float32)
    expect = [0, 0, 1, 0, 0, 1, 1, 1]
    g = len(c)
    p = SimpleNamespace(**_operands(np.tile(c, (3, 1)), np.arange(g), g))
    X = torch.tensor(x[None], device=DEV)
    keys, probe = _run(ext, p, X)
    _, kref, pref = _reference(p, X)
    want = sum(bit << i for i, bit in enumerate(expect))
    assert int(keys[0]) == want == int(kref[0])
    assert torch.equal(probe, pref) and probe.tolist() == [1, want]


@pytest.mark.parametrize("b,d,g", SHAPES)
def test_varying_probe_every_group_varies(ext, b, d, g):
    p = _problem(b, d, g, seed=7, constant=False)
    keys, probe = _run(ext, p, p.X)
    _, kref, pref = _reference(p, p.X)
    assert torch.equal(keys, kref) and torch.equal(probe, pref)
    assert bool((keys == (1 << g) - 1).all())
    assert probe.tolist() == [1, (1 << g) - 1]


# ----------------------------------------------------------------------- #
# all_same

def _same_rows(b, differs=None):
    """B copies of one row whose constant groups are all close; row
    ``differs`` gets one constant column pushed out of tolerance."""
    p = _problem(1, 50, 12, seed=3)
    bgc = p.bg_min.clone()
    row = torch.where(torch.tensor(p.const_cols, device=DEV), bgc, p.X[0])
    X = row[None].repeat(b, 1).contiguous()
    if differs is not None:
        j = int(np.nonzero(p.const_cols)[0][0])
        X[differs, j] = bgc[j] + 1.0
    return p, X


@pytest.mark.parametrize("b,differs,same", [
    (257, None, 1), (257, 256, 0), (257, 0, 0), (1, None, 1)])
def test_varying_probe_all_same(ext, b, differs, same):
    p, X = _same_rows(b, differs)
    keys, probe = _run(ext, p, X)
    _, kref, pref = _reference(p, X)
    assert torch.equal(keys, kref) and torch.equal(probe, pref)
    assert int(probe[0]) == same
    assert int(probe[1]) == int(kref[0])
    if differs is not None:
        assert int((keys != keys[(differs + 1) % b]).sum()) == 1


def test_varying_probe_reused_buffers_alternate(ext):
    """Three calls into the same output buffers with answers true / false /
    true: nothing of a call survives into the next."""
    b = 257
    p, same = _same_rows(b)
    _, diff = _same_rows(b, differs=b - 1)
    keys = torch.full((b,), -1, dtype=torch.int64, device=DEV)
    probe = torch.full((2,), -1, dtype=torch.int64, device=DEV)
    seen = []
    for X in (same, diff, same):
        _run(ext, p, X, keys, probe)
        _, kref, pref = _reference(p, X)
        assert torch.equal(keys, kref) and torch.equal(probe, pref)
        seen.append(int(probe[0]))
    assert seen == [1, 0, 1]


def test_varying_probe_rejects_more_than_62_groups(ext):
    p = _problem(2, 70, 62, seed=1)
    p.n_groups = 63
    with pytest.raises(RuntimeError, match="varying_probe"):
        _run(ext, p, p.X)


# ----------------------------------------------------------------------- #
# engine

def _engine(pred, bg, groups, dtype, device="cuda"):
    from distributedkernelshap_amd.config import KernelConfig
    from distributedkernelshap_amd.core.engine import KernelShapEngine

    return KernelShapEngine(
        pred, bg, groups=groups, link="logit", seed=0, device=device,
        kernels=KernelConfig(predict_dtype=dtype),
    )


@pytest.mark.parametrize("pinned", [False, True])
def test_engine_probe_eager_capture_replay_reject_and_mixed(pinned):
    from distributedkernelshap_amd.models import LinearPredictor, make_adult_like

    data = make_adult_like(n_instances=8, n_background=100, seed=12)
    pred = LinearPredictor.random(data.X.shape[1], 2, seed=12)
    cols = np.asarray(data.groups[2])
    bg = data.background.copy()
    bg[:, cols] = bg[0, cols]               # constant background columns
    Xa = data.X.copy()
    Xa[:, cols] = bg[0, cols] + 1.0         # group 2 varies for everyone
    Xb = data.X.copy()
    Xb[:, cols] = bg[0, cols]               # ... for no one
    Xc = Xa.copy()
    Xc[:4, cols] = bg[0, cols]              # two patterns in one batch

    def feed(X):
        if not pinned:
            return X
        return torch.from_numpy(X.astype(np.float32)).pin_memory()

    e32 = _engine(pred, bg, data.groups, "fp32")
    e64 = _engine(pred, bg, data.groups, "fp64")
    gpu = e32._gpu
    r1 = e32.shap_values(feed(Xa))          # eager
    assert gpu._spec is None
    r2 = e32.shap_values(feed(Xa))          # capture
    assert gpu._spec is not None and len(gpu._graphs) == 1
    r3 = e32.shap_values(feed(Xa))          # speculative replay
    assert gpu._spec is not None
    r4 = e32.shap_values(feed(Xb))          # speculation rejected
    assert gpu._spec is None
    r5 = e32.shap_values(feed(Xc))          # two buckets
    fresh4 = _engine(pred, bg, data.groups, "fp32").shap_values(feed(Xb))
    fresh5 = _engine(pred, bg, data.groups, "fp32").shap_values(feed(Xc))
    ref = {k: e64.shap_values(X) for k, X in (("a", Xa), ("b", Xb), ("c", Xc))}
    for o in range(2):
        assert r1[o].dtype == r3[o].dtype == np.float64
        assert r3[o].flags["C_CONTIGUOUS"]
        assert np.allclose(r1[o], r2[o], atol=1e-6)
        assert np.allclose(r1[o], r3[o], atol=1e-6)
        assert np.array_equal(r4[o], fresh4[o])
        assert np.allclose(r5[o], fresh5[o], atol=1e-6)
        assert np.all(r4[o][:, 2] == 0.0) and np.all(r5[o][:4, 2] == 0.0)
        assert np.all(r5[o][4:, 2] != 0.0) and np.all(r1[o][:, 2] != 0.0)
        for r, k in ((r1, "a"), (r2, "a"), (r3, "a"), (r4, "b"), (r5, "c")):
            err = np.abs(r[o] - ref[k][o]).max()
            print(f"call on X{k} class {o}: max err vs fp64 = {err:.3e}")
            assert err < 1e-3


def test_engine_probe_serves_the_tree_bucketing_path():
    """A non-linear predictor has no speculative path: its calls go through
    the bucketing branch, two patterns here, on the shared probe."""
    from distributedkernelshap_amd.core.engine import KernelShapEngine
    from distributedkernelshap_amd.models import TreeEnsemblePredictor

    d = 8
    rng = np.random.Generator(np.random.Philox(key=[73, 8]))
    bg, X = rng.normal(size=(30, d)), rng.normal(size=(4, d))
    bg[:, 3] = 0.7                 # constant background column ...
    X[1, 3] = 0.7                  # ... that instance 1 matches: 7 varying
    pred = TreeEnsemblePredictor.random(d, 2, trees=20, depth=3)
    sv_cpu = KernelShapEngine(
        pred, bg, link="logit", seed=0, device="cpu").shap_values(X)
    gpu = KernelShapEngine(pred, bg, link="logit", seed=0, device="cuda")
    sv = gpu.shap_values(X)
    g = gpu._gpu
    assert g.trees_fused is True
    keys, probe = g._varying_probe(
        torch.tensor(X, dtype=torch.float32, device=DEV))
    assert keys.tolist() == [255, 255 - 8, 255, 255]
    assert probe.tolist() == [0, 255]
    for o in range(2):
        assert sv[o][1, 3] == 0.0
        assert np.allclose(sv[o], sv_cpu[o], atol=5e-4, rtol=5e-3), \
            np.abs(sv[o] - sv_cpu[o]).max()
