"""predict_backends.blend_ey_f64 on CPU tensors against a triple Python loop
in numpy fp64: the sentinel column, the chunking over samples and the
weighted background mean."""
import numpy as np
import pytest
import torch

from distributedkernelshap_amd.ops.predict_backends import blend_ey_f64

B, S, N, D, N_OUT = 2, 5, 3, 6, 2
# four groups over six columns; groups 1 (two columns) and 3 vary, groups 0
# and 2 (two columns) do not and read the always-off sentinel column m = 2
COL_GROUP = np.array([0, 1, 1, 2, 2, 3])
VARYING = [1, 3]
WIDTH = 6
ROW_BYTES = 8 * 3 * B * N * WIDTH        # the chunk formula's bytes per sample


@pytest.fixture(scope="module")
def problem():
    rng = np.random.default_rng(7)
    masks = rng.integers(0, 2, size=(B, S, len(VARYING))).astype(np.uint8)
    masks[0, 0] = 0                      # all off: pure background rows
    masks[1, 1] = 1                      # all on: every varying column from x
    X = rng.normal(size=(B, D))
    bg = rng.normal(size=(N, D))
    wbg = rng.random(N)
    wbg /= wbg.sum()
    A = rng.normal(size=(N_OUT, D))
    c = rng.normal(size=N_OUT)
    vmap = np.full(4, len(VARYING))
    vmap[VARYING] = np.arange(len(VARYING))
    colk = vmap[COL_GROUP]
    assert colk.tolist() == [2, 0, 0, 2, 2, 1]

    ref = np.zeros((B, S, N_OUT))
    for b in range(B):
        for s in range(S):
            on = np.append(masks[b, s], 0)[colk].astype(bool)
            for n in range(N):
                row = np.where(on, X[b], bg[n])
                ref[b, s] += wbg[n] / (1.0 + np.exp(-(A @ row + c)))

    At, ct = torch.from_numpy(A), torch.from_numpy(c)

    def run(**kw):
        return blend_ey_f64(
            torch.from_numpy(masks), torch.from_numpy(X),
            torch.from_numpy(bg), torch.from_numpy(wbg),
            torch.from_numpy(colk),
            lambda rows: torch.sigmoid(rows @ At.T + ct), N_OUT, WIDTH, **kw)

    return run, ref


def test_blend_matches_numpy_loop_at_every_chunking(problem):
    run, ref = problem
    one = run()                                   # default budget: one chunk
    assert one.shape == (B, S, N_OUT) and one.dtype == torch.float64
    outs = {
        "s_chunk=1": run(budget_bytes=ROW_BYTES),
        "s_chunk=2": run(budget_bytes=2 * ROW_BYTES),   # chunks of 2, 2, 1
        "one chunk": one,
    }
    for name, ey in outs.items():
        err = np.abs(ey.numpy() - ref).max()
        print(f"blend_ey_f64 {name}: max|ey - loop| = {err:.3e} bound=1e-14")
        assert err <= 1e-14, name
    # a sample's arithmetic does not depend on the chunk it falls into
    assert torch.equal(outs["s_chunk=1"], one)
    assert torch.equal(outs["s_chunk=2"], one)


def test_blend_budget_below_one_sample_still_runs_one_per_chunk(problem):
    run, ref = problem
    assert np.abs(run(budget_bytes=1).numpy() - ref).max() <= 1e-14
