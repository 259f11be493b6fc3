"""Fl-trust on the GPU: plato_agg_trust_stats and plato_agg_scaled_sum against the numpy restatements
(tests/fltrust_oracle.py), and the engine and hook against the reference fixtures (tests/golden/fltrust_*).

Shape of the statistics kernel (plato_amd/csrc/trust.hip) that the sizes below walk around: workgroups of
256 lanes take 512 coordinates per pass and 8 clients per batch; a chunk is PLATO_AGG_TRUST_TILE = 1,024
coordinates for models this small, one workgroup per (chunk, batch); the int64 region has chunks of its
own.  The client counts and the coordinate counts are independent grid dimensions: every coordinate count
is run at the small K, the large K at a few of them.

The statistics are compared with the exact sums (math.fsum of the exact float64 products) within
property (c) of the header: D * 2^-53 * sum|terms|.  The scaled sum is compared bit for bit.
"""

import asyncio
import types

import numpy as np
import pytest
import torch

from plato_amd import _lib
from plato_amd.engine import FedAvgEngine
from plato_amd.multi import MultiDeviceEngine
from plato_amd.servers import TrustAggregationMixin, make_server
from tests import fltrust_cases as fc
from tests import fltrust_oracle as fo
from tests.test_fltrust import (CASES, NAMES, bits, case_of, check_cosines_against_fixture,
                                check_output_against_fixture, inputs)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TILE = _lib.PLATO_AGG_TRUST_TILE
KS_SMALL = (1, 2, 3, 7, 8, 9)          # +-1 around the 8-client batch
KS_LARGE = (64, 65, 128, 255, 256)
NS = (1, 3, 255, 256, 257, 511, 512, 513, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 0)
NS_LARGE_K = (3, 257, TILE + 1, 2 * TILE + 1)
NIS = (0, 1, 5)
SENTINEL = -7.0
EPS = np.float32(1e-9)


@pytest.fixture(scope="module")
def engine():
    return FedAvgEngine(DEV)


def tables(xf: np.ndarray, xi: np.ndarray, order=None):
    k, n_f, n_i = xf.shape[0], xf.shape[1], xi.shape[1]
    order = range(k) if order is None else order
    df = torch.from_numpy(np.ascontiguousarray(xf)).to(DEV)
    di = torch.from_numpy(np.ascontiguousarray(xi)).to(DEV)
    tf = torch.tensor([df.data_ptr() + 4 * n_f * c for c in order], dtype=torch.int64, device=DEV)
    ti = torch.tensor([di.data_ptr() + 8 * n_i * c for c in order], dtype=torch.int64, device=DEV)
    return (df, di), tf, ti


def device_stats(xf, xi, ref, eps=EPS, order=None) -> np.ndarray:
    """plato_agg_trust_stats on [K, n] host matrices and a reference vector [n_f + n_i]; the output is
    sentinel-filled and 64 guard elements follow the output and the workspace: the kernels write their
    own elements and nothing else."""
    n_f, n_i = xf.shape[1], xi.shape[1]
    keep, tf, ti = tables(xf, xi, order)
    rf = torch.from_numpy(np.ascontiguousarray(ref[:n_f])).to(DEV)
    ri = torch.from_numpy(np.ascontiguousarray(ref[n_f:])).to(DEV)
    got = launch_stats(tf, ti, rf, ri, eps, n_f, n_i)
    del keep
    return got


def launch_stats(tf, ti, rf, ri, eps, n_f: int, n_i: int) -> np.ndarray:
    """device_stats on pointer tables and reference halves that are on the device already, with the same
    guards."""
    k = tf.numel()
    nbytes = _lib.lib().plato_agg_trust_stats_workspace(k, n_f, n_i)
    assert nbytes >= (3 * k + 1) * 8
    words = (nbytes + 7) // 8
    work = torch.full((words + 64,), SENTINEL, dtype=torch.float64, device=DEV)
    out = torch.full((3 * k + 1 + 64,), SENTINEL, dtype=torch.float64, device=DEV)
    _lib.call("plato_agg_trust_stats", tf.data_ptr() if n_f else None, ti.data_ptr() if n_i else None, k,
              rf.data_ptr() if n_f else None, ri.data_ptr() if n_i else None, float(eps), n_f, n_i, work.data_ptr(),
              out.data_ptr(), torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    assert bool((out[3 * k + 1:] == SENTINEL).all()) and bool((work[words:] == SENTINEL).all())
    return out[: 3 * k + 1].cpu().numpy()


def device_mean(xf, xi, order=None):
    n_f, n_i = xf.shape[1], xi.shape[1]
    keep, tf, ti = tables(xf, xi, order)
    out_f = torch.zeros(n_f + 4, device=DEV)
    out_i = torch.zeros(n_i + 4, device=DEV)
    _lib.call("plato_agg_mean_rows", tf.data_ptr() if n_f else None, ti.data_ptr() if n_i else None, tf.numel(),
              out_f.data_ptr() if n_f else None, out_i.data_ptr() if n_i else None, n_f, n_i,
              torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    del keep
    return np.concatenate([out_f[:n_f].cpu().numpy(), out_i[:n_i].cpu().numpy()])


def device_scaled_sum(xf, xi, mul, div, post, order=None):
    n_f, n_i = xf.shape[1], xi.shape[1]
    keep, tf, ti = tables(xf, xi, order)
    k = tf.numel()
    scal = torch.from_numpy(np.concatenate([np.float32(mul), np.float32(div)])).to(DEV)
    out_f = torch.full((n_f + 64,), SENTINEL, device=DEV)
    out_i = torch.full((n_i + 64,), SENTINEL, device=DEV)
    _lib.call("plato_agg_scaled_sum", tf.data_ptr() if n_f else None, ti.data_ptr() if n_i else None, k,
              scal.data_ptr(), scal.data_ptr() + 4 * k, float(post), out_f.data_ptr() if n_f else None,
              out_i.data_ptr() if n_i else None, n_f, n_i, torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    assert bool((out_f[n_f:] == SENTINEL).all()) and bool((out_i[n_i:] == SENTINEL).all())
    del keep
    return np.concatenate([out_f[:n_f].cpu().numpy(), out_i[:n_i].cpu().numpy()])


def clients(rng, k: int, n_f: int, n_i: int):
    """A common model plus noise, some rows negated (dots of both signs), counters nearby."""
    base = rng.standard_normal(n_f).astype(np.float32)
    xf = (base + np.float32(0.25) * rng.standard_normal((k, n_f)).astype(np.float32)).astype(np.float32)
    xf[1::3] = -xf[1::3]
    xi = rng.integers(0, 10001, n_i, dtype=np.int64) + rng.integers(0, 9, (k, n_i), dtype=np.int64)
    ref = np.concatenate([base, rng.standard_normal(n_i).astype(np.float32) * np.float32(5000)]).astype(np.float32)
    return xf, xi, ref


def assert_stats(got, xf, xi, ref, eps=EPS):
    exp, mag = fo.stats(fo.columns(xf, xi), ref, eps)
    d = xf.shape[1] + xi.shape[1]
    err = np.abs(got - exp)
    assert np.all(err <= d * 2.0 ** -53 * mag), float(np.max(err / np.maximum(mag, 1e-300)))


def sizes_of(k):
    ns = NS if k in KS_SMALL else NS_LARGE_K
    for at, n_f in enumerate(ns):
        for n_i in ((NIS[at % 3],) if n_f else (1, 5)):
            yield n_f, n_i


# ------------------------------------------------------------------ plato_agg_trust_stats
@pytest.mark.parametrize("k", KS_SMALL + KS_LARGE)
def test_stats_are_within_property_c_of_the_exact_sums_and_repeat_bitwise(k):
    rng = np.random.default_rng(7000 + k)
    for n_f, n_i in sizes_of(k):
        xf, xi, ref = clients(rng, k, n_f, n_i)
        got = device_stats(xf, xi, ref)
        assert_stats(got, xf, xi, ref)
        assert np.array_equal(bits(got), bits(device_stats(xf, xi, ref)))


@pytest.mark.parametrize("k", (3, 9, 65, 256))
def test_a_permuted_table_gives_the_permuted_output(k):
    rng = np.random.default_rng(7100 + k)
    for n_f, n_i in ((2 * TILE + 1, 5), (257, 0)):
        xf, xi, ref = clients(rng, k, n_f, n_i)
        got = device_stats(xf, xi, ref)
        perm = rng.permutation(k)
        moved = device_stats(xf, xi, ref, order=perm)
        for part in range(3):
            assert np.array_equal(bits(moved[part * k:(part + 1) * k]), bits(got[part * k:(part + 1) * k][perm]))
        assert bits(moved[3 * k:]) == bits(got[3 * k:])


def test_a_clients_values_do_not_depend_on_k():
    rng = np.random.default_rng(7200)
    xf, xi, ref = clients(rng, 65, 2 * TILE + 1, 5)
    big, small = device_stats(xf, xi, ref), device_stats(xf[:3], xi[:3], ref)
    for part in range(3):
        assert np.array_equal(bits(big[part * 65:part * 65 + 3]), bits(small[part * 3:part * 3 + 3]))
    assert bits(big[-1:]) == bits(small[-1:])
    # nor on the batch the client falls in: row 0 moved to slot 64
    order = list(range(1, 65)) + [0]
    moved = device_stats(xf, xi, ref, order=order)
    assert [bits(moved[p * 65 + 64:p * 65 + 65])[0] for p in range(3)] == [bits(big[p * 65:p * 65 + 1])[0] for p in range(3)]


def test_special_values_follow_ieee_and_stay_in_their_row():
    rng = np.random.default_rng(7300)
    k, n_f, n_i = 9, TILE + 1, 5
    xf, xi, ref = clients(rng, k, n_f, n_i)
    clean = device_stats(xf, xi, ref)
    xf[4, TILE] = np.nan          # the last coordinate of the second chunk
    xf[6, 17] = np.inf
    got = device_stats(xf, xi, ref)
    rows = lambda r: [r, k + r, 2 * k + r]  # noqa: E731
    assert np.isnan(got[rows(4)]).all()
    assert got[k + 6] == np.inf and got[2 * k + 6] == np.inf and np.isinf(got[6])
    assert got[6] == (np.inf if ref[17] > 0 else -np.inf)
    others = [j for r in range(k) if r not in (4, 6) for j in rows(r)] + [3 * k]
    assert np.array_equal(bits(got[others]), bits(clean[others]))
    # an inf in r poisons every dot, no norm; inf - inf across two coordinates is NaN
    ref2 = ref.copy()
    ref2[3] = np.inf
    got = device_stats(xf[:3], xi[:3], ref2)
    assert np.isinf(got[:3]).all() and got[9] == np.inf and np.isfinite(got[3:9]).all()
    ref2[5] = -np.inf if xf[0, 5] * xf[0, 3] > 0 else np.inf
    assert np.isnan(device_stats(xf[:3], xi[:3], ref2)[0])


def test_counters_are_promoted_with_round_to_nearest_even():
    xi = np.array([[(1 << 25) + 1, (1 << 25) + 3], [-(1 << 25) - 1, 5], [(1 << 25) + 2, (1 << 24) + 1]], dtype=np.int64)
    ref = np.array([1.0, 2.0], dtype=np.float32)
    for xf, r in ((np.zeros((3, 0), dtype=np.float32), ref),
                  (np.ones((3, 3), dtype=np.float32), np.concatenate([np.zeros(3, dtype=np.float32), ref]))):
        got = device_stats(xf, xi, r, eps=np.float32(0))
        c = xi.astype(np.float32).astype(np.float64)  # 2^25 + 1 -> 2^25, 2^25 + 3 -> 2^25 + 4, 2^24 + 1 -> 2^24
        assert c[0, 0] == 2.0 ** 25 and c[0, 1] == 2.0 ** 25 + 4 and c[2, 1] == 2.0 ** 24
        assert np.array_equal(got[:3], c @ ref.astype(np.float64))
        assert np.array_equal(got[3:6], (c * c).sum(axis=1) + xf.shape[1])
        assert np.array_equal(got[6:9], got[3:6])  # eps = 0


def test_the_eps_shift_is_one_fp32_addition():
    rng = np.random.default_rng(7400)
    k, n_f = 3, 513
    xf = (rng.standard_normal((k, n_f)) * 1e-6).astype(np.float32)  # fp32(x + 1e-9) != x at this size
    xf[2] = np.float32(3.0)                                       # ... and == x here
    xi = np.zeros((k, 0), dtype=np.int64)
    ref = rng.standard_normal(n_f).astype(np.float32)
    got = device_stats(xf, xi, ref)
    assert_stats(got, xf, xi, ref)
    assert got[2 * k] != got[k] and got[2 * k + 1] != got[k + 1]
    assert got[2 * k + 2] == got[k + 2]
    shifted = (xf + EPS).astype(np.float32).astype(np.float64)
    assert abs(got[2 * k] - float((shifted[0] ** 2).sum())) <= n_f * 2.0 ** -53 * float((shifted[0] ** 2).sum())
    # the eps argument is honoured
    other = device_stats(xf, xi, ref, eps=np.float32(0.5))
    assert_stats(other, xf, xi, ref, eps=np.float32(0.5))
    assert np.array_equal(bits(other[:2 * k]), bits(got[:2 * k])) and other[2 * k] != got[2 * k]


def test_stats_of_the_device_mean_feed_the_references_cosines():
    """mean_rows -> trust_stats, as the engine chains them: the restatement's mean has the same bits."""
    rng = np.random.default_rng(7500)
    xf, xi, _ = clients(rng, 9, 2 * TILE + 1, 5)
    mean = device_mean(xf, xi)
    assert np.array_equal(bits(mean), bits(fo.mean(xf, xi)))
    assert_stats(device_stats(xf, xi, mean), xf, xi, mean)


# ------------------------------------------------------------------ plato_agg_scaled_sum
def scalars(rng, k):
    mul = rng.random(k).astype(np.float32)
    mul[rng.random(k) < 0.3] = 0.0
    mul[rng.random(k) < 0.1] *= np.float32(-1.0)
    div = (rng.random(k) * 50 + 0.01).astype(np.float32)
    return mul, div, np.float32(rng.random() * 40 + 0.1)


@pytest.mark.parametrize("k", KS_SMALL + KS_LARGE)
def test_scaled_sum_equals_the_restatement_bit_for_bit(k):
    rng = np.random.default_rng(8000 + k)
    for n_f, n_i in sizes_of(k):
        xf, xi, _ = clients(rng, k, n_f, n_i)
        mul, div, post = scalars(rng, k)
        got = device_scaled_sum(xf, xi, mul, div, post)
        assert np.array_equal(bits(got), bits(fo.scaled_sum(fo.columns(xf, xi), mul, div, post)))


def test_scaled_sum_special_values():
    rng = np.random.default_rng(8100)
    k, n_f, n_i = 5, 257, 3
    xf, xi, _ = clients(rng, k, n_f, n_i)
    mul, div, post = scalars(rng, k)
    mul[2] = 0.0
    xf[2, 5] = np.inf                 # 0 * inf = NaN: the row is read although its weight is 0
    xf[:, 6] = 0.0
    xf[1::2, 6] = -0.0                # signed zeros: +0 + -0 = +0
    xf[:, 7] = -0.0
    mul[0] = -0.0                     # -0 * -0 = +0
    xf[:, 8] = np.float32(1e-38)      # subnormal products and quotients
    xf[3, 9] = np.nan
    xi[0, 0] = (1 << 25) + 1
    got = device_scaled_sum(xf, xi, mul, div, post)
    exp = fo.scaled_sum(fo.columns(xf, xi), mul, div, post)
    assert np.isnan(got[5]) and np.isnan(got[9]) and not bits(got[6:7]).any()
    assert 0 < abs(exp[8]) < np.finfo(np.float32).tiny * 64
    both = ~np.isnan(exp)
    assert np.array_equal(np.isnan(got), np.isnan(exp)) and np.array_equal(bits(got[both]), bits(exp[both]))
    # subnormal quotients: tiny elements over a large divisor, then scaled back up
    xf = np.full((2, 65), np.float32(3e-38))
    xf[1] = np.float32(-7e-39)
    xi = np.zeros((2, 0), dtype=np.int64)
    mul, div, post = np.float32([1.0, 0.5]), np.float32([1024.0, 3.0]), np.float32(2.0 ** 20)
    got = device_scaled_sum(xf, xi, mul, div, post)
    exp = fo.scaled_sum(xf, mul, div, post)
    assert np.array_equal(bits(got), bits(exp)) and np.all(exp != 0)
    # an infinite divisor, a zero divisor, an infinite post
    mul, div = np.float32([1.0, 1.0]), np.float32([np.inf, 0.0])
    xf = np.float32([[1.0, 0.0, -2.0], [1.0, 0.0, -2.0]])
    got = device_scaled_sum(xf, xi, mul, div, np.float32(1.0))
    exp = fo.scaled_sum(xf, mul, div, np.float32(1.0))
    assert got[0] == np.inf and np.isnan(got[1]) and got[2] == -np.inf
    assert np.array_equal(np.isnan(got), np.isnan(exp))


def test_scaled_sum_follows_the_table_order():
    rng = np.random.default_rng(8200)
    k = 33
    xf, xi, _ = clients(rng, k, 513, 1)
    mul, div, post = scalars(rng, k)
    perm = rng.permutation(k)
    got = device_scaled_sum(xf, xi, mul, div, post, order=perm)
    exp = fo.scaled_sum(fo.columns(xf, xi)[perm], mul, div, post)  # scalar j belongs to table slot j
    assert np.array_equal(bits(got), bits(exp))


# ------------------------------------------------------------------ engine and hook
def _flat(layout, result):
    got_f, got_i, dtypes = fc.flat_result(layout, result)
    assert dtypes == ["torch.float32"]  # the counters too
    assert list(result) == [e.name for e in layout.entries]
    for e in layout.entries:
        assert tuple(result[e.name].shape) == tuple(e.shape)
    return np.concatenate([got_f, got_i])


def _check(name, out, scal, order=None):
    """The engine's output against the restatement fed the device's own statistics (bit for bit) and
    against the reference fixture (within the CPU tests' bounds)."""
    case = case_of(name)
    _, xf, xi, cols = inputs(name)
    k = cols.shape[0]
    order = list(range(k)) if order is None else list(order)
    for key in ("dots", "norms", "norms_eps", "cos", "weights", "div"):
        assert scal[key].dtype == np.float32 and scal[key].shape == (k,)
    exp = fo.scaled_sum(cols[order], scal["weights"], scal["div"], scal["nm"])
    assert np.array_equal(bits(out), bits(exp))
    if order == list(range(k)):
        # the device's statistics against the restatement's, through the scalars they give
        mine = fo.fltrust(xf, xi)[1]
        assert np.allclose(scal["cos"], mine["cos"], rtol=0, atol=16 * 2.0 ** -24)
        ratio = check_output_against_fixture(case, out, scal, cols)
        err = check_cosines_against_fixture(case, scal)
        print(f"{name}: output within {ratio:.4f} of the bound, max |cos - cos_ref| {err:.3e}")
    if case["recipe"]["mirror"]:
        assert not bits(out).any()  # all +0


@pytest.mark.parametrize("name", NAMES)
def test_engine_equals_the_restatement_and_is_within_the_bounds_of_the_reference(engine, name):
    layout, xf, xi, _ = inputs(name)
    payloads = fc.state_dicts(layout, xf.copy(), xi.copy())  # the shared inputs stay read-only
    got = engine.aggregate_fltrust(payloads)
    _check(name, _flat(layout, got), engine.last_trust)


@pytest.mark.parametrize("name", NAMES)
def test_round_launch_fltrust_with_an_order(engine, name):
    layout, xf, xi, _ = inputs(name)
    payloads = fc.state_dicts(layout, xf.copy(), xi.copy())  # the shared inputs stay read-only
    k = len(payloads)
    rnd = engine.begin(payloads[0], k)
    rnd.deltas = False
    for i, p in enumerate(payloads):
        rnd.put_client(i, p)
    rnd.launch_fltrust()
    _check(name, _flat(layout, rnd.result()), rnd.trust)
    t = rnd.timings
    assert t["mean_rows_ms"] > 0 and t["trust_stats_ms"] > 0 and t["trust_combine_ms"] > 0
    assert t["trust_scalars_ms"] > 0 and t["kernel_ms"] > 0
    assert rnd.algorithmic_bytes() == (3 * k + 1) * layout.n_f32 * 4 + 3 * k * layout.n_i64 * 8 + layout.n_i64 * 4
    order = list(np.random.default_rng(k).permutation(k))
    rnd.launch_fltrust(order=order)
    _check(name, _flat(layout, rnd.result()), rnd.trust, order)


class _Base:
    """What the hook needs of a Plato server."""


@pytest.mark.parametrize("name", NAMES)
def test_hook_equals_the_reference(name):
    layout, xf, xi, _ = inputs(name)
    payloads = fc.state_dicts(layout, xf.copy(), xi.copy())  # the shared inputs stay read-only
    server = make_server(base=_Base, mixin=TrustAggregationMixin)()
    server.secure_aggregation_type, server.aggregation_device = "Fl-trust", "cuda:0"
    updates = [types.SimpleNamespace(report=types.SimpleNamespace(num_samples=10)) for _ in payloads]
    got = asyncio.run(server.aggregate_weights(updates, payloads[0], payloads))
    _check(name, _flat(layout, got), server.aggregation_engine().last_trust)
    t = server._plato_amd_timings
    assert t["trust_stats_ms"] > 0 and t["trust_combine_ms"] > 0
    assert server.get_logged_items()["aggregation_kernel_ms"] > 0


def test_refusals():
    layout, xf, xi, _ = inputs("fltrust_lenet5_k8")
    payloads = fc.state_dicts(layout, xf.copy(), xi.copy())  # the shared inputs stay read-only
    eng = FedAvgEngine(DEV)
    eng.delta_arenas = True
    rnd = eng.begin(payloads[0], len(payloads))
    rnd.put_baseline(payloads[0])
    for i, p in enumerate(payloads):
        rnd.put_client(i, p)
    with pytest.raises(ValueError, match="holds deltas"):
        rnd.launch_fltrust()
    bf16 = [type(p)((n, t.to(torch.bfloat16)) for n, t in p.items()) for p in payloads]
    with pytest.raises(ValueError, match="native payloads"):
        FedAvgEngine(DEV).aggregate_fltrust(bf16)
    eng = FedAvgEngine(DEV)
    rnd = eng.begin(payloads[0], len(bf16), codec="bf16")  # the template is the (native) baseline
    for i, p in enumerate(bf16):
        rnd.put_client(i, p)
    with pytest.raises(ValueError, match="native payloads"):
        rnd.launch_fltrust()
    with pytest.raises(ValueError, match="at most 256 clients, got 257"):
        FedAvgEngine(DEV).aggregate_fltrust([payloads[0]] * 257)
    eng = FedAvgEngine(DEV)
    rnd = eng.begin(payloads[0], 257)
    rnd.deltas = False
    for i in range(257):
        rnd.put_client(i, payloads[i % len(payloads)])
    with pytest.raises(ValueError, match="at most 256 clients, got 257"):
        rnd.launch_fltrust()
    with pytest.raises(ValueError, match="no client payloads"):
        FedAvgEngine(DEV).aggregate_fltrust([])
    eng = FedAvgEngine(DEV)
    eng.layout_align = "fedadp"
    with pytest.raises(ValueError, match="no alignment padding"):
        eng.aggregate_fltrust(payloads)
    with pytest.raises(NotImplementedError, match="one GPU"):
        MultiDeviceEngine(["cuda:0", "cuda:0"]).aggregate_fltrust(payloads)
    assert len(CASES) == 6
