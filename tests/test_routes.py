"""ops/routes.py: the boundaries of the kernel-routing tables, on plain
Python values (no GPU, no torch)."""
from types import SimpleNamespace

import pytest

from distributedkernelshap_amd.ops import routes


def _kc(predict_dtype="fp32", fused_predict=True, wls_mode="auto"):
    return SimpleNamespace(predict_dtype=predict_dtype,
                           fused_predict=fused_predict, wls_mode=wls_mode)


def test_default_kernel_config_has_the_routed_fields():
    from distributedkernelshap_amd.config import KernelConfig

    kc = KernelConfig()
    assert (kc.predict_dtype, kc.fused_predict, kc.wls_mode) == (
        "fp32", True, "auto")
    assert routes.linear_predict_route(kc, 12, 100, 2, True) == ("u8", False)


def test_pad_m_pad_n():
    assert [routes.pad_m(m) for m in range(1, 6)] == [4, 4, 4, 4, 8]
    assert routes.pad_m(64) == 64 and routes.pad_m(65) == 68
    assert routes.pad_n(16) == 16 and routes.pad_n(17) == 32
    assert routes.pad_n(100) == 112 and routes.pad_n(128) == 128


# (kc kwargs, m, N, n_out, act3) -> (route, pairwise)
PREDICT_CASES = [
    (dict(), 64, 100, 2, False, ("u8", False)),
    (dict(), 65, 100, 2, False, ("tiled", False)),
    (dict(), 12, 128, 2, False, ("u8", False)),
    (dict(), 12, 129, 2, False, ("tiled", False)),
    (dict(), 12, 100, 3, False, ("torch", False)),
    (dict(fused_predict=False), 12, 100, 2, False, ("torch", False)),
    (dict(predict_dtype="bf16"), 32, 100, 2, False, ("bf16", False)),
    (dict(predict_dtype="bf16"), 33, 100, 2, False, ("tiled_bf16", False)),
    # 2 x 4 images x 128 x 40 bf16 = 81,920 B > 64 KiB of LDS
    (dict(predict_dtype="bf16x2"), 40, 100, 4, False, ("tiled", False)),
    (dict(predict_dtype="bf16x2"), 40, 100, 2, True, ("tiled_bf16", True)),
    (dict(predict_dtype="bf16"), 40, 100, 4, False, ("tiled_bf16", False)),
    # the pairwise flag follows act3 on every tiled / torch route only
    (dict(), 12, 100, 2, True, ("u8", False)),
    (dict(predict_dtype="bf16"), 12, 100, 2, True, ("bf16", False)),
    (dict(), 65, 100, 2, True, ("tiled", True)),
    (dict(fused_predict=False), 12, 100, 2, True, ("torch", True)),
    # the bf16 kernel needs one column tile as well
    (dict(predict_dtype="bf16"), 12, 129, 2, False, ("tiled_bf16", False)),
]


@pytest.mark.parametrize("kw,m,N,n_out,act3,expected", PREDICT_CASES)
def test_linear_predict_route(kw, m, N, n_out, act3, expected):
    assert routes.linear_predict_route(_kc(**kw), m, N, n_out, act3) == expected


@pytest.mark.parametrize("mode,m,n_out,expected", [
    ("auto", 15, 2, "kernel"),
    ("auto", 24, 2, "kernel"),
    ("auto", 25, 2, "gram"),
    ("auto", 513, 2, "gram"),
    ("auto", 514, 2, "torch"),
    ("auto", 10, 9, "torch"),
    ("auto", 9, 8, "kernel"),
    ("torch", 15, 2, "torch"),
    ("generic", 24, 2, "kernel"),
    ("generic", 30, 2, "torch"),
    ("mfma", 30, 2, "gram"),
])
def test_wls_route(mode, m, n_out, expected):
    assert routes.wls_route(_kc(wls_mode=mode), m, n_out) == expected


_PACKED_BASE = dict(kc=_kc(), linear=True, m=15, N=100, n_out=2,
                    l1_active=False)


def test_packed_ok_inside_the_envelope():
    assert routes.packed_ok(**_PACKED_BASE) is True
    assert routes.packed_ok(**dict(_PACKED_BASE, m=2)) is True
    assert routes.packed_ok(**dict(_PACKED_BASE, m=13, n_out=4)) is True
    assert routes.packed_ok(**dict(_PACKED_BASE, m=16, n_out=1)) is True
    assert routes.packed_ok(**dict(_PACKED_BASE, N=128)) is True
    assert routes.packed_ok(**dict(_PACKED_BASE, kc=_kc(wls_mode="mfma")))


@pytest.mark.parametrize("change", [
    dict(linear=False),
    dict(kc=_kc(predict_dtype="bf16")),
    dict(kc=_kc(fused_predict=False)),
    dict(kc=_kc(wls_mode="generic")),
    dict(m=1),
    dict(m=65, n_out=1),
    dict(N=129),
    dict(n_out=3),
    dict(m=16),                       # 15 + 2 > 16
    dict(l1_active=True),
], ids=lambda c: ",".join(c))
def test_packed_ok_fails_one_condition_at_a_time(change):
    assert routes.packed_ok(**dict(_PACKED_BASE, **change)) is False


def test_graph_ok_is_packed_ok_without_dtype_and_solve_limits():
    base = dict(_PACKED_BASE)
    assert routes.graph_ok(**base)
    # the two conditions packed_ok adds
    assert routes.graph_ok(**dict(base, m=16))
    assert routes.graph_ok(**dict(base, m=64))
    assert routes.graph_ok(**dict(base, kc=_kc(predict_dtype="bf16x2")))
    # everything else is shared
    for change in (dict(linear=False), dict(kc=_kc(fused_predict=False)),
                   dict(kc=_kc(wls_mode="torch")), dict(m=1), dict(m=65),
                   dict(N=129), dict(n_out=8), dict(l1_active=True)):
        assert not routes.graph_ok(**dict(base, **change)), change


def test_graph_body_and_eager_loop_disagree_only_in_the_named_gap():
    """Inside ``graph_ok`` and outside ``packed_ok`` the captured body and
    the eager loop pick the same kernel, except under a bf16 dtype with
    33..64 varying groups: the discrepancy routes.py names."""
    assert list(routes.GRAPH_EAGER_BF16_GAP) == list(range(33, 65))
    for dtype in ("fp32", "bf16", "bf16x2"):
        kc = _kc(predict_dtype=dtype)
        for m in range(2, 65):
            for n_out in (1, 2, 4):
                graph = routes.graph_predict_route(kc, m, n_out)
                eager, _ = routes.linear_predict_route(kc, m, 100, n_out, False)
                if dtype != "fp32" and m in routes.GRAPH_EAGER_BF16_GAP:
                    assert graph == "u8" and eager.startswith("tiled")
                else:
                    assert graph == eager, (dtype, m, n_out)


@pytest.mark.parametrize("m,N,n_out,expected", [
    (64, 100, 2, "u8"), (65, 100, 2, "torch"), (12, 128, 4, "u8"),
    (12, 129, 2, "torch"), (12, 100, 3, "torch"),
])
def test_sharded_predict_route(m, N, n_out, expected):
    assert routes.sharded_predict_route(m, N, n_out) == expected
