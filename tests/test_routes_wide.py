"""ops/routes.py: the envelope of the wide linear predict kernel and the
output chunks of the WLS solve, on plain Python values (no GPU, no torch)."""
from types import SimpleNamespace

import pytest

from distributedkernelshap_amd.ops import routes


def _kc(predict_dtype="fp32", fused_predict=True, wls_mode="auto"):
    return SimpleNamespace(predict_dtype=predict_dtype,
                           fused_predict=fused_predict, wls_mode=wls_mode)


@pytest.mark.parametrize("n_out,expected", [
    (2, False), (3, True), (4, False), (5, True), (8, True), (9, True),
    (16, True), (17, False),
])
def test_wide_linear_ok_output_counts(n_out, expected):
    assert routes.wide_linear_ok(_kc(), 12, 100, n_out) is expected


@pytest.mark.parametrize("m,expected", [
    (1, False), (2, True), (64, True), (65, False),
])
def test_wide_linear_ok_varying_groups(m, expected):
    assert routes.wide_linear_ok(_kc(), m, 100, 10) is expected


@pytest.mark.parametrize("N,expected", [
    (1, True), (300, True), (512, True), (513, False),
])
def test_wide_linear_ok_background_rows(N, expected):
    assert routes.wide_linear_ok(_kc(), 12, N, 10) is expected


@pytest.mark.parametrize("kw,expected", [
    (dict(), True),
    (dict(predict_dtype="bf16"), True),
    (dict(predict_dtype="bf16x2"), True),
    (dict(predict_dtype="fp64"), False),
    (dict(fused_predict=False), False),
])
def test_wide_linear_ok_kernel_config(kw, expected):
    assert routes.wide_linear_ok(_kc(**kw), 12, 100, 10) is expected


def test_pad_out():
    assert [routes.pad_out(o) for o in (3, 4, 5, 8, 9, 10, 12, 13, 16)] == [
        4, 4, 8, 8, 12, 12, 12, 16, 16]


@pytest.mark.parametrize("linear,n_out,expected", [
    (True, 8, [(0, 8)]),
    (True, 9, [(0, 8), (8, 9)]),
    (True, 16, [(0, 8), (8, 16)]),
    (True, 17, [(0, 17)]),
    (False, 10, [(0, 10)]),
    (True, 3, [(0, 3)]),
])
def test_wls_output_chunks(linear, n_out, expected):
    chunks = routes.wls_output_chunks(linear, n_out)
    assert chunks == expected
    # every chunk is within the kernels' 8 outputs wherever chunking applies
    if len(chunks) > 1:
        assert all(hi - lo <= 8 for lo, hi in chunks)
        assert [routes.wls_route(_kc(), 12, hi - lo) for lo, hi in chunks] == [
            "kernel", "kernel"]


def test_existing_routes_keep_their_answers_for_wide_counts():
    kc = _kc()
    assert routes.linear_predict_route(kc, 12, 100, 3, False) == ("torch", False)
    assert routes.sharded_predict_route(12, 100, 3) == "torch"
    assert routes.wls_route(kc, 10, 9) == "torch"
    assert not routes.graph_ok(kc, True, 12, 100, 10, False)
    assert not routes.packed_ok(kc, True, 12, 100, 3, False)
