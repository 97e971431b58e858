"""The float64 reference that the u8-mask predict kernels are held to
(tests/linear_predict_reference.py), itself checked against a plain triple
loop in numpy on one tiny shape. Needs no GPU."""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from linear_predict_reference import (  # noqa: E402
    column_bound, derived_tolerance, fp64_reference, lipschitz,
)


def _loop_reference(masks, diff, base, w, act, n_out):
    b_, s_, m_ = masks.shape
    oimg, n_ = base.shape
    ey = np.zeros((b_, s_, n_out))
    for b in range(b_):
        for s in range(s_):
            for n in range(n_):
                z = [base[o, n] + sum(diff[b, o, k, n] for k in range(m_)
                                      if masks[b, s, k])
                     for o in range(oimg)]
                if act == 0:
                    p = z
                elif act == 1:
                    p = [1.0 / (1.0 + math.exp(-v)) for v in z]
                elif act == 2:
                    e = [math.exp(v - max(z)) for v in z]
                    p = [v / sum(e) for v in e]
                else:
                    p = [1.0 / (1.0 + math.exp(z[0])),
                         1.0 / (1.0 + math.exp(-z[0]))]
                for o in range(n_out):
                    ey[b, s, o] += w[n] * p[o]
    return ey


@pytest.mark.parametrize("n_out,act", [(1, 0), (2, 1), (3, 2), (2, 2), (2, 3)])
def test_reference_matches_triple_loop(n_out, act):
    rng = np.random.Generator(np.random.Philox(key=[3, act]))
    b, s, m, kpad, n = 2, 5, 3, 4, 6
    oimg = 1 if act == 3 else n_out
    masks = rng.integers(0, 2, size=(b, s, m)).astype(np.uint8)
    diff = rng.normal(size=(b, oimg, kpad, n))
    diff[:, :, m:] = 99.0               # k slots past m are not part of z
    base = rng.normal(size=(oimg, n))
    w = rng.uniform(0.1, 1.0, size=n)   # non-uniform, does not sum to 1
    z, p, ey = fp64_reference(
        torch.tensor(masks), torch.tensor(diff), torch.tensor(base),
        torch.tensor(w), act)
    assert z.dtype == p.dtype == ey.dtype == torch.float64
    assert ey.shape == (b, s, n_out) and p.shape == (b, s, n_out, n)
    want = _loop_reference(masks, diff, base, w, act, n_out)
    assert np.abs(ey.numpy() - want).max() < 1e-13


def test_reference_act3_keeps_saturated_p0():
    """p0 = sigmoid(-z), not 1 - p1: at z = 40 it is 4e-18, not 0."""
    masks = torch.ones(1, 1, 1, dtype=torch.uint8)
    diff = torch.full((1, 1, 1, 1), 10.0, dtype=torch.float64)
    base = torch.full((1, 1), 30.0, dtype=torch.float64)
    _, _, ey = fp64_reference(masks, diff, base, torch.ones(1), 3)
    assert ey[0, 0, 0].item() == pytest.approx(math.exp(-40.0), rel=1e-12)
    assert ey[0, 0, 1].item() == pytest.approx(1.0, rel=1e-12)


def test_derived_tolerance_formula():
    diff = torch.tensor([[[[1.0, -2.0], [0.5, 3.0]]]])      # (1,1,2,2)
    base = torch.tensor([[0.25, -1.0]])
    w = torch.tensor([0.5, -0.25])
    assert column_bound(diff, base) == 6.0                  # |-1| + 2 + 3
    assert (lipschitz(1, 0), lipschitz(2, 1), lipschitz(2, 2),
            lipschitz(2, 3), lipschitz(4, 2)) == (1.0, 0.25, 0.25, 0.25, 0.5)
    p = torch.tensor([0.5, -2.0])
    tol = derived_tolerance(diff, base, w, p, n=2, n_out=1, act=0, k_terms=4)
    want = 5 * 2.0 ** -24 * 6.0 + 6 * 2.0 ** -24 * 0.75 * 2.0 + 1e-6
    assert tol == pytest.approx(want, rel=1e-12)
