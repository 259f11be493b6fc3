"""Fl-trust without a GPU: the host scalars (plato_amd.trust) and the numpy restatement of the pipeline
(tests/fltrust_oracle.py) against the reference fixtures (tests/golden/fltrust_*), the hook's dispatch
on a stub engine, and the host-side argument checks of plato_agg_trust_stats / plato_agg_scaled_sum.

Bounds (both from the reference's own error and the number formats, never from the code under test):

* output, per coordinate: |out - ref| <= sum_k |c_k[e]| * (|g_k - g_k^ref| + (2K + 4) * 2^-24 *
  max(|g_k|, |g_k^ref|)) + 3K * 2^-149 with g = w_k / div_k * nm in float64 from each side's fp32
  scalars: three roundings per term and any-order fp32 summation on both sides.
* cosines: |cos_k - cos_k^ref| <= ref_self_err[k] + mean_order_shift[k] + 16 * 2^-24: the reference's own
  fp32 dot / norm error and the shift from its mean's summation order (both float64 figures of the
  fixture), plus this side's few fp32 roundings.
"""

import asyncio
import functools
import os
import types

import numpy as np
import pytest

from plato_amd import _lib
from plato_amd.trust import fltrust_weights, weights_from_scalars
from tests import fltrust_cases as fc
from tests import fltrust_oracle as fo

CASES = fc.load_cases()
NAMES = [c["recipe"]["name"] for c in CASES]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def case_of(name):
    return next(c for c in CASES if c["recipe"]["name"] == name)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(layout, xf, xi, promoted columns) of a fixture case; computed once, shared, never modified."""
    layout, xf, xi = fc.build_inputs(case_of(name)["recipe"])
    cols = fo.columns(xf, xi)
    for a in (xf, xi, cols):
        a.setflags(write=False)
    return layout, xf, xi, cols


@functools.lru_cache(maxsize=None)
def restated(name):
    """(output, scalars) of the numpy restatement of a fixture case."""
    _, xf, xi, _ = inputs(name)
    out, scal = fo.fltrust(xf, xi)
    out.setflags(write=False)
    return out, scal


@functools.lru_cache(maxsize=None)
def full_arrays():
    return fc.load_full()


def check_output_against_fixture(case, out, scal, cols):
    """``out`` [D] (fp32 region, then int64 region) within the output bound of the reference's values.
    Returns the largest |out - ref| / bound met."""
    g, g_ref = fo.gains(scal), fo.gains(fc.reference_scalars(case))
    worst = 0.0
    n_f32 = inputs(case["recipe"]["name"])[0].n_f32
    for region, idx, ref in fc.reference_values(case, full_arrays()):
        at = idx if region == "f32" else idx + n_f32
        bound = fo.output_bound(cols[:, at], g, g_ref)
        err = np.abs(out[at].astype(np.float64) - ref.astype(np.float64))
        assert np.all(err <= bound), (case["recipe"]["name"], region, float(np.max(err / bound)))
        worst = max(worst, float(np.max(err / bound)))
    return worst


def check_cosines_against_fixture(case, scal):
    exp = case["expected"]
    ref = fc.reference_scalars(case)
    lim = np.array(exp["ref_self_err"]) + np.array(exp["mean_order_shift"]) + 16 * 2.0 ** -24
    err = np.abs(scal["cos"].astype(np.float64) - ref["cos"].astype(np.float64))
    assert np.all(err <= lim), (case["recipe"]["name"], float(np.max(err / lim)))
    return float(np.max(err))


# ------------------------------------------------------------------ the host scalars
@pytest.mark.parametrize("name", NAMES)
def test_weights_from_the_references_dots_and_norms_are_the_references_bit_for_bit(name):
    case = case_of(name)
    ref, k = fc.reference_scalars(case), case["recipe"]["k"]
    cos, weights = weights_from_scalars(ref["dots"], ref["norms"], ref["nm"])
    assert np.array_equal(bits(cos), bits(ref["cos"]))
    assert np.array_equal(bits(weights), bits(ref["weights"]))
    # through the float64 statistics: the square of an fp32 norm is exact in float64 and so is its root
    d = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    stats = np.concatenate([d(ref["dots"]), d(ref["norms"]) ** 2, d(ref["norms_eps"]) ** 2, [float(ref["nm"]) ** 2]])
    scal = fltrust_weights(stats, k)
    for key in ("dots", "norms", "norms_eps", "cos", "weights", "div"):
        assert scal[key].dtype == np.float32 and scal[key].shape == (k,)
        assert np.array_equal(bits(scal[key]), bits(ref[key])), key
    assert isinstance(scal["nm"], np.float32) and bits(scal["nm"]) == bits(ref["nm"])
    clipped = np.maximum(scal["cos"], np.float32(0))
    assert np.array_equal(bits(clipped), bits(ref["clipped"]))


def test_the_fixture_clips_clients_where_the_recipe_intends_it():
    counts = {c["recipe"]["name"]: int(np.sum(fc.reference_scalars(c)["cos"] < 0)) for c in CASES}
    for c in CASES:
        assert counts[c["recipe"]["name"]] >= len(c["recipe"]["negate"])
    assert counts["fltrust_lenet5_k8"] >= 2 and counts["fltrust_lenet5_k33"] >= 3
    assert counts["fltrust_lenet5_k64"] >= 13 and counts["fltrust_resnet18_k8"] >= 2
    mirror = fc.reference_scalars(case_of("fltrust_lenet5_k2"))
    assert not bits(mirror["cos"]).any() and not bits(mirror["weights"]).any()


def test_a_nan_cosine_makes_every_weight_nan():
    stats = np.array([1.0, np.nan, 2.0, 4.0, 4.0, 4.0, 4.0, 4.0, 4.0, 9.0])
    scal = fltrust_weights(stats, 3)
    assert np.isnan(scal["cos"][1]) and not np.isnan(scal["cos"][[0, 2]]).any()
    assert np.isnan(scal["weights"]).all()
    # a NaN norm of one client does the same
    stats = np.array([1.0, 1.0, 2.0, 4.0, np.nan, 4.0, 4.0, 4.0, 4.0, 9.0])
    assert np.isnan(fltrust_weights(stats, 3)["weights"]).all()


def test_cosines_all_at_or_below_zero_give_zero_weights():
    stats = np.array([-1.0, 0.0, -3.0, 4.0, 4.0, 4.0, 4.0, 4.0, 4.0, 9.0])
    scal = fltrust_weights(stats, 3)
    assert np.all(scal["cos"] <= 0)
    assert not bits(scal["weights"]).any()  # max(cos, 0) = +0, and +0 / (0 + 1e-9) = +0


def test_one_client_needs_no_special_case():
    scal = fltrust_weights(np.array([4.0, 4.0, 4.0, 4.0]), 1)  # x = m, |x| = 2
    assert scal["cos"][0] == np.float32(1.0) and scal["weights"][0] == np.float32(1.0)
    assert scal["nm"] == np.float32(2.0) and scal["div"][0] == np.float32(2.0)
    with pytest.raises(ValueError, match="doubles"):
        fltrust_weights(np.zeros(5), 1)
    with pytest.raises(ValueError, match="doubles"):
        fltrust_weights(np.zeros(1), 0)


def test_the_norm_of_a_squared_norm_beyond_fp32_is_finite():
    scal = fltrust_weights(np.array([1.0, 1e40, 1e40, 1e40]), 1)
    assert np.isfinite(scal["norms"][0]) and scal["norms"][0] == np.float32(1e20)


# ------------------------------------------------------------------ the restatement against the reference
@pytest.mark.parametrize("name", NAMES)
def test_restatement_is_within_the_bounds_of_the_reference(name):
    case = case_of(name)
    out, scal = restated(name)
    cols = inputs(name)[3]
    assert out.dtype == np.float32 and out.shape == (cols.shape[1],)
    ratio = check_output_against_fixture(case, out, scal, cols)
    err = check_cosines_against_fixture(case, scal)
    print(f"{name}: output within {ratio:.4f} of the bound, max |cos - cos_ref| {err:.3e}")
    assert case["expected"]["dtypes"] == ["torch.float32"]
    if case["recipe"]["mirror"]:
        assert not bits(out).any()  # all +0
        ref = fc.reference_values(case, full_arrays())
        assert all(not bits(v).any() for _, _, v in ref)


def test_scaled_sum_restatement_does_three_roundings_and_a_true_division():
    cols = np.array([[3.0, 1e-30, -0.0, np.inf], [7.0, 5.0, 0.0, 1.0]], dtype=np.float32)
    mul, div, post = np.float32([0.1, 0.0]), np.float32([3.0, 7.0]), np.float32(1.7)
    got = fo.scaled_sum(cols, mul, div, post)
    t = np.float32(np.float32(np.float32(np.float32(3.0) * mul[0]) / div[0]) * post)
    assert got[0] == t  # row 1 adds 7 * 0 = +0
    assert got[3] == np.inf  # inf * 0.1, then + 1 * 0
    assert np.isnan(fo.scaled_sum(cols, mul[::-1].copy(), div, post)[3])  # mul = 0 against the inf element
    assert not bits(fo.scaled_sum(cols[:, 2:3], mul, div, post)).any()  # +0 + -0 = +0


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
        self.log.append(("launch_robust", mode, trim))

    def launch_multi_krum(self, f=2, order=None):
        self.log.append(("launch_multi_krum", f))

    def launch_bulyan(self, f, order=None):
        self.log.append(("launch_bulyan", f))

    def launch_fltrust(self, order=None):
        self.log.append(("launch_fltrust",))

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


def _server(kind, **attrs):
    import torch

    from plato_amd.servers import TrustAggregationMixin

    s = type("Server", (TrustAggregationMixin,), {"secure_aggregation_type": kind, **attrs})()
    s._plato_amd_engine = _Engine()
    updates = [types.SimpleNamespace(report=types.SimpleNamespace(num_samples=n)) for n in (1, 3)]
    payloads = [{"w": torch.zeros(2)}, {"w": torch.ones(2)}]
    return s, updates, payloads


def _run(s, updates, payloads):
    return asyncio.run(s.aggregate_weights(updates, payloads[0], payloads))


def test_hook_fltrust_launches_and_releases_arrivals():
    s, updates, payloads = _server("Fl-trust")
    assert _run(s, updates, payloads) == {"w": 1}
    assert s._plato_amd_engine.log == ["client", "client", ("launch_fltrust",)]
    assert s._plato_amd_engine.released == 1


def test_hook_hands_every_other_name_to_its_parents():
    for kind, attrs, last in (("Median", {}, ("launch_robust", "median", 0)),
                              ("Multi-krum", {}, ("launch_multi_krum", 2)),
                              ("Bulyan", {"num_attackers": 3}, ("launch_bulyan", 3)),
                              ("Trimmed-mean", {}, ("launch_robust", "nearest_mean", 0))):
        s, updates, payloads = _server(kind, **attrs)
        assert _run(s, updates, payloads) == {"w": 1}
        assert s._plato_amd_engine.log == ["client", "client", last]
        assert s._plato_amd_engine.released == 1
    s, updates, payloads = _server(None)  # the reference's "Fedavg is applied" branch
    s.robust_aggregation_type = lambda: None
    assert _run(s, updates, payloads) == {"w": 1}
    assert s._plato_amd_engine.log[-1] == ("launch", [0.25, 0.75])


@pytest.mark.parametrize("name", ["Krum", "Afa", "fl-trust", "Fltrust"])
def test_hook_refuses_unknown_names_without_touching_the_engine(name):
    s, updates, payloads = _server(name)
    with pytest.raises(ValueError, match="supported: Bulyan, Fl-trust, Median, Multi-krum, Trimmed-mean"):
        _run(s, updates, payloads)
    assert s._plato_amd_engine.log == [] and s._plato_amd_engine.released == 0


def test_the_parents_keep_refusing_fltrust():
    import torch

    from plato_amd.servers import DetectorAggregationMixin, RobustAggregationMixin

    for mixin in (RobustAggregationMixin, DetectorAggregationMixin):
        s = type("Server", (mixin,), {"secure_aggregation_type": "Fl-trust"})()
        s._plato_amd_engine = _Engine()
        with pytest.raises(ValueError, match="'Fl-trust' is not supported on the GPU"):
            asyncio.run(s.aggregate_weights([], {"w": torch.zeros(2)}, [{"w": torch.zeros(2)}]))
        assert s._plato_amd_engine.log == []


def test_hook_refuses_several_devices_and_coded_payloads_before_any_engine_call():
    import torch

    s, updates, payloads = _server("Fl-trust")
    s._plato_amd_engine.primary = object()  # what a multi-GPU engine carries
    with pytest.raises(NotImplementedError, match="one GPU"):
        _run(s, updates, payloads)
    assert s._plato_amd_engine.log == [] and s._plato_amd_engine.released == 0
    s, updates, payloads = _server("Fl-trust")
    coded = [{"w": torch.zeros(2, dtype=torch.bfloat16)}, {"w": torch.ones(2, dtype=torch.bfloat16)}]
    with pytest.raises(ValueError, match="native payloads"):
        _run(s, updates, coded)
    assert s._plato_amd_engine.log == []


def test_multi_device_engine_refuses_fltrust():
    from plato_amd.multi import MultiDeviceEngine, MultiRound

    with pytest.raises(NotImplementedError, match="one GPU"):
        MultiDeviceEngine.aggregate_fltrust(object(), [])
    with pytest.raises(NotImplementedError, match="one GPU"):
        MultiRound.launch_fltrust(object())


# ------------------------------------------------------------------ ABI
def test_trust_argument_errors_are_raised_without_gpu_work():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = _lib.lib()
    a = 1 << 12  # an aligned non-null address: nothing is dereferenced on these paths
    assert _lib.ABI_VERSION == 5 and lib.plato_agg_abi_version() == 5
    tile = _lib.PLATO_AGG_TRUST_TILE
    ws = lib.plato_agg_trust_stats_workspace
    assert ws(0, 64, 0) == 0 and ws(257, 64, 0) == 0 and ws(-1, 64, 0) == 0
    assert ws(4, 1 << 38, 0) == 0 and ws(4, 0, 1 << 38) == 0
    assert ws(4, 0, 0) == 256
    assert ws(4, 1, 0) == 13 * 8 and ws(4, tile, 1) == 2 * 13 * 8 and ws(256, tile + 1, 0) == 2 * 769 * 8
    assert ws(1, 1024 * tile, 0) == 1024 * 4 * 8 and ws(1, 1024 * tile + 1, 0) == 513 * 4 * 8  # chunks of two tiles

    # trust_stats: (x_f32, x_i64, K, ref_f32, ref_i64, eps, n_f32, n_i64, workspace, out, stream)
    stats = lambda *args: _lib.call("plato_agg_trust_stats", *args, None)  # noqa: E731
    for k in (0, 257, -3):
        with pytest.raises(ValueError, match=r"K must be in 1\.\.256"):
            stats(a, None, k, a, None, 1e-9, 64, 0, a, a)
    for args in ((None, None, 4, a, None, 1e-9, 64, 0, a, a), (a, None, 4, None, None, 1e-9, 64, 0, a, a)):
        with pytest.raises(ValueError, match="null fp32"):
            stats(*args)
    for args in ((a, None, 4, a, a, 1e-9, 64, 1, a, a), (a, a, 4, a, None, 1e-9, 64, 1, a, a)):
        with pytest.raises(ValueError, match="null int64"):
            stats(*args)
    for args in ((a, None, 4, a, None, 1e-9, 64, 0, None, a), (a, None, 4, a, None, 1e-9, 64, 0, a, None)):
        with pytest.raises(ValueError, match="null output or workspace"):
            stats(*args)
    with pytest.raises(ValueError, match="8-byte aligned"):
        stats(a + 4, None, 4, a, None, 1e-9, 64, 0, a, a)
    with pytest.raises(ValueError, match="8-byte aligned"):
        stats(a, a + 4, 4, a, a, 1e-9, 64, 1, a, a)
    with pytest.raises(ValueError, match="4-byte aligned"):
        stats(a, None, 4, a + 2, None, 1e-9, 64, 0, a, a)
    with pytest.raises(ValueError, match="16-byte aligned"):
        stats(a, None, 4, a, None, 1e-9, 64, 0, a, a + 8)
    with pytest.raises(ValueError, match="256-byte aligned"):
        stats(a, None, 4, a, None, 1e-9, 64, 0, a + 128, a)
    with pytest.raises(ValueError, match="2\\^38"):
        stats(a, None, 4, a, None, 1e-9, 1 << 38, 0, a, a)
    stats(None, None, 4, None, None, 1e-9, 0, 0, a, a)  # nothing to do: no launch, no error

    # scaled_sum: (x_f32, x_i64, K, mul, div, post, out_f32, out_i64, n_f32, n_i64, stream)
    ssum = lambda *args: _lib.call("plato_agg_scaled_sum", *args, None)  # noqa: E731
    for k in (0, 257, -3):
        with pytest.raises(ValueError, match=r"K must be in 1\.\.256"):
            ssum(a, None, k, a, a, 1.0, a, None, 64, 0)
    for args in ((None, None, 4, a, a, 1.0, a, None, 64, 0), (a, None, 4, a, a, 1.0, None, None, 64, 0)):
        with pytest.raises(ValueError, match="null fp32"):
            ssum(*args)
    for args in ((a, None, 4, a, a, 1.0, a, a, 64, 1), (a, a, 4, a, a, 1.0, a, None, 64, 1)):
        with pytest.raises(ValueError, match="null int64"):
            ssum(*args)
    for args in ((a, None, 4, None, a, 1.0, a, None, 64, 0), (a, None, 4, a, None, 1.0, a, None, 64, 0)):
        with pytest.raises(ValueError, match="null scalar table"):
            ssum(*args)
    with pytest.raises(ValueError, match="8-byte aligned"):
        ssum(a + 4, None, 4, a, a, 1.0, a, None, 64, 0)
    with pytest.raises(ValueError, match="scalar tables must be 4-byte aligned"):
        ssum(a, None, 4, a + 2, a, 1.0, a, None, 64, 0)
    with pytest.raises(ValueError, match="16-byte aligned"):
        ssum(a, None, 4, a, a, 1.0, a + 4, None, 64, 0)
    with pytest.raises(ValueError, match="16-byte aligned"):
        ssum(a, a, 4, a, a, 1.0, a, a + 2, 64, 1)
    with pytest.raises(ValueError, match="2\\^38"):
        ssum(a, a, 4, a, a, 1.0, a, a, 64, 1 << 38)
    ssum(None, None, 4, a, a, 1.0, None, None, 0, 0)  # nothing to do: no launch, no error
