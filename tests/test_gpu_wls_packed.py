"""wls_solve_packed (K7p), one wave per instance: against the fp64 CPU solve
and against the unchanged u8-path kernel ``ext.wls_solve`` on the same masks
with broadcast weights. The packed kernel keeps every entry's operation order,
so the two kernels are expected to agree bit for bit; the bound asserted is
the looser one that reordered fp32 sums would still meet."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

DEV = "cuda"


@pytest.fixture(scope="module")
def ext():
    from distributedkernelshap_amd.ops import load_extension

    return load_extension()


CASES = [
    (5, 500, 12, 2, 14),     # the existing shape
    (3, 24, 4, 1, 4),        # fewer than 64 samples: one partial block
    (3, 257, 12, 2, 12),     # a tail of one sample
    (2, 2072, 12, 2, 12),    # the benchmark's chunk count and 24-sample tail
    (3, 300, 2, 8, 3),       # a 1x1 system
    (3, 300, 15, 2, 15),     # full 16-column tile
    (3, 300, 9, 8, 9),       # full 16-column tile
    (1, 64, 16, 1, 16),      # M = 16: bit 15 is the eliminated feature
    (7, 130, 5, 4, 9),       # n_out = 4
    (2, 100, 6, 3, 8),       # n_out between two instantiations
]


@pytest.mark.parametrize("b,s,m,n_out,G", CASES)
def test_wls_solve_packed_cases(ext, b, s, m, n_out, G):
    from distributedkernelshap_amd.core.solver import solve_wls

    g = torch.Generator(device=DEV).manual_seed(11 + s + m)
    masks = (torch.rand(b, s, m, generator=g, device=DEV) > 0.5).to(torch.uint8)
    masks[:, :, 0] = (torch.rand(b, s, generator=g, device=DEV) > 0.3).to(torch.uint8)
    kw = torch.rand(s, generator=g, device=DEV) + 0.05
    ey = torch.randn(b, s, n_out, generator=g, device=DEV)
    total = torch.randn(b, n_out, generator=g, device=DEV)
    packed = torch.empty(b, s, dtype=torch.int64, device=DEV)
    ext.pack_masks(masks, packed)
    rng = np.random.Generator(np.random.Philox(key=[G, m]))
    varying = np.sort(rng.choice(G, size=m, replace=False)).tolist()
    skipped = [i for i in range(G) if i not in varying]
    vidx = torch.tensor(varying, dtype=torch.int64, device=DEV)

    phi_full = torch.full((b, G, n_out), float("nan"), device=DEV)
    ext.wls_solve_packed(packed, kw, ey, total, vidx, phi_full)
    assert not bool(torch.isnan(phi_full).any())

    kwb = kw[None].expand(b, s).contiguous()
    phi_old = torch.empty(b, m, n_out, device=DEV)
    ext.wls_solve(masks, kwb, ey, total, phi_old, packed)

    ref = np.stack([
        solve_wls(
            masks[i].cpu().numpy(), kw.double().cpu().numpy(),
            ey[i].double().cpu().numpy(), total[i].double().cpu().numpy())
        for i in range(b)
    ])
    ph = phi_full.cpu().numpy()
    err_new = np.abs(ph[:, varying] - ref).max()
    err_old = np.abs(phi_old.cpu().numpy() - ref).max()
    same = torch.equal(phi_full[:, vidx], phi_old)
    print(f"wls packed (b={b} s={s} m={m} n_out={n_out}): err_new={err_new:.3e} "
          f"err_old={err_old:.3e} bit-identical to wls_solve: {same}")
    assert err_new <= 2.0 * err_old
    assert np.all(ph[:, skipped] == 0.0)
    assert np.allclose(ph.sum(axis=1), total.cpu().numpy(), atol=1e-4)
