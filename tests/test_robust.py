"""Robust aggregation on the CPU: the numpy restatement against the reference fixtures, the host-side
argument checks of plato_agg_robust_columns, and the hook's dispatch (engine = test double).

The device side of the same cases is tests/test_robust_gpu.py.
"""

import asyncio
import os
import types

import numpy as np
import pytest

from plato_amd import _lib
from tests import robust_cases as rc
from tests import robust_oracle as ro

CASES = rc.load_cases()


@pytest.fixture(scope="module")
def full():
    return rc.load_full()


def check_against_fixture(case, got_f, got_i, xf, full=None):
    """Bitwise on every coordinate but the listed mixed-zero ones (by value), after canon."""
    recipe, exp = case["recipe"], case["expected"]
    mz = recipe["mixed_zero"]
    assert len(mz) <= 4
    # the exclusion hides nothing: no other column holds both zero signs around a zero median
    found = rc.mixed_zero_columns(xf, ro.median_columns(xf))
    assert set(found) <= set(mz), found
    for j in mz:  # by value
        assert got_f[j] == 0.0
    cf, ci = rc.canon_case(got_f, mz), rc.canon(got_i)
    assert rc.sha(cf) == exp["sha_f32"]
    assert rc.sha(ci) == exp["sha_i64f"]
    for j, bits in exp["samples_f32"]:
        assert "%08x" % int(cf.view(np.uint32)[j]) == bits, j
    for j, bits in exp["samples_i64f"]:
        assert "%08x" % int(ci.view(np.uint32)[j]) == bits, j
    if full is not None and recipe["name"] + ".f32" in full.files:
        assert cf.tobytes() == full[recipe["name"] + ".f32"].tobytes()


def test_fixture_set_is_the_one_the_generator_writes(full):
    assert [c["recipe"]["k"] for c in CASES if c["recipe"]["model"] == "lenet5"] == list(rc.KS_LENET)
    assert [c["recipe"]["k"] for c in CASES if c["recipe"]["model"] == "resnet18"] == [8]
    assert sorted(full.files) == sorted(f"median_lenet5_k{k}.f32" for k in rc.FULL_KS)
    for c in CASES:
        assert c["expected"]["dtypes"] == ["torch.float32"]  # the counters too


@pytest.mark.parametrize("case", CASES, ids=[c["recipe"]["name"] for c in CASES])
def test_restatement_equals_the_reference_median(case, full):
    layout, xf, xi = rc.build_inputs(case["recipe"])
    got_f, got_i = ro.median(xf, xi)
    check_against_fixture(case, got_f, got_i, xf, full)
    # the special columns did what they were made for
    k = case["recipe"]["k"]
    assert np.isnan(got_f[0])
    assert got_f[4] == np.float32(1.5) and got_f[5] == np.float32(0.5)
    assert 0 < abs(float(got_f[3])) < np.finfo(np.float32).tiny  # a subnormal survives (no flush to zero)
    if xi.size:
        srt = np.sort(xi[:, 0])[(k - 1) // 2]
        assert srt > 1 << 24 and got_i[0] == np.float32(srt) and float(got_i[0]) != float(srt)


def test_restatement_orders_zeros_infinities_and_nans():
    neg0, pos0 = np.float32(-0.0), np.float32(0.0)
    x = np.array([[pos0, np.inf, 1.0, np.nan], [neg0, -np.inf, np.inf, np.nan], [neg0, -np.inf, -np.inf, np.nan],
                  [pos0, np.inf, np.inf, np.nan]], dtype=np.float32)
    out = ro.median_columns(x)
    assert np.signbit(out[0]) and out[0] == 0  # K = 4: index 1 of (-0, -0, +0, +0)
    assert out[1] == -np.inf and out[2] == np.float32(1.0) and np.isnan(out[3])
    big = np.array([[(1 << 24) + 1], [-(1 << 24) - 1], [(1 << 53) + 1]], dtype=np.int64)
    assert ro.median_columns(big)[0] == np.float32(1 << 24)  # 2^24 + 1 rounds to even


def test_argument_errors_are_raised_without_gpu_work():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    a = 1 << 12  # an aligned non-null address: nothing is dereferenced on these paths
    call = lambda *args: _lib.call("plato_agg_robust_columns", *args)  # noqa: E731
    with pytest.raises(ValueError, match=r"K must be in 1\.\.256"):
        call(0, a, None, 0, 0, a, None, 64, 0, None)
    with pytest.raises(ValueError, match=r"K must be in 1\.\.256"):
        call(0, a, None, 257, 0, a, None, 64, 0, None)
    with pytest.raises(ValueError, match="mode"):
        call(2, a, None, 4, 0, a, None, 64, 0, None)
    with pytest.raises(ValueError, match="trim"):
        call(0, a, None, 4, 2, a, None, 64, 0, None)
    with pytest.raises(ValueError, match="trim"):
        call(0, a, None, 4, -1, a, None, 64, 0, None)
    with pytest.raises(ValueError, match="aligned"):
        call(0, a, None, 4, 0, a + 4, None, 64, 0, None)
    with pytest.raises(ValueError, match="aligned"):
        call(0, a + 4, None, 4, 0, a, None, 64, 0, None)
    with pytest.raises(ValueError, match="null"):
        call(0, None, None, 4, 0, a, None, 64, 0, None)
    with pytest.raises(ValueError, match="null int64"):
        call(0, a, None, 4, 0, a, a, 64, 1, None)
    assert _lib.ABI_VERSION == 5 and _lib.lib().plato_agg_abi_version() == 5


# ------------------------------------------------------------------ hook dispatch (stub engine)
class _Round:
    def __init__(self, log):
        self.log, self.timings = log, {}

    def put_baseline(self, b):
        self.log.append("baseline")

    def adopt(self, slot, p):
        return False

    def put_client(self, slot, p):
        self.log.append("client")

    def launch(self, weights, scales=None):
        self.log.append(("launch", list(weights)))

    def launch_robust(self, mode, trim=0):
        self.log.append(("launch_robust", mode))

    def wait(self):
        pass

    def result(self):
        return {"w": 1}

    def algorithmic_bytes(self):
        return 0


class _Engine:
    def __init__(self):
        self.log, self.released = [], 0

    def begin(self, template, k, codec="native"):
        return _Round(self.log)

    def release_arrivals(self):
        self.released += 1


def _server(kind):
    import torch

    from plato_amd.servers import RobustAggregationMixin

    s = type("Server", (RobustAggregationMixin,), {"secure_aggregation_type": kind})()
    s._plato_amd_engine = _Engine()
    updates = [types.SimpleNamespace(report=types.SimpleNamespace(num_samples=n)) for n in (1, 3)]
    payloads = [{"w": torch.zeros(2)}, {"w": torch.ones(2)}]
    return s, updates, payloads


def test_hook_without_a_key_is_the_fused_fedavg():
    s, updates, payloads = _server(None)
    assert s.robust_aggregation_type() is None  # Plato absent or the key unset
    assert asyncio.run(s.aggregate_weights(updates, payloads[0], payloads)) == {"w": 1}
    assert s._plato_amd_engine.log == ["baseline", "client", "client", ("launch", [0.25, 0.75])]
    assert s._plato_amd_engine.released == 1


def test_hook_median_launches_the_robust_kernel_and_releases_arrivals():
    s, updates, payloads = _server("Median")
    assert asyncio.run(s.aggregate_weights(updates, payloads[0], payloads)) == {"w": 1}
    assert s._plato_amd_engine.log == ["client", "client", ("launch_robust", "median")]
    assert s._plato_amd_engine.released == 1


def test_hook_refuses_other_aggregators():
    s, updates, payloads = _server("Krum")
    with pytest.raises(ValueError, match="Median"):
        asyncio.run(s.aggregate_weights(updates, payloads[0], payloads))
    assert s._plato_amd_engine.log == []
