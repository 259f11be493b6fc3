"""Robust aggregation on the GPU: plato_agg_robust_columns against the reference fixtures (bit for bit,
mixed-zero columns by value) and against the numpy restatement (tests/robust_oracle.py)."""

import asyncio
import types

import numpy as np
import pytest
import torch

from plato_amd import _lib, workloads
from plato_amd.arena import ArenaLayout
from plato_amd.engine import ClientSlab, DeviceArena, FedAvgEngine
from plato_amd.servers import RobustAggregationMixin
from plato_amd.synthetic import fill_baseline, fill_clients
from tests import robust_cases as rc
from tests import robust_oracle as ro
from tests.test_robust import check_against_fixture

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CASES = rc.load_cases()
KS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256)


@pytest.fixture(scope="module")
def engine():
    return FedAvgEngine(DEV)


@pytest.fixture(scope="module")
def full():
    return rc.load_full()


def device_median(xf: np.ndarray, xi: np.ndarray):
    """plato_agg_robust_columns on [K, n] host matrices; (fp32 region, int64 region as fp32) as numpy."""
    k = xf.shape[0]
    n_f, n_i = xf.shape[1], xi.shape[1]
    df = torch.from_numpy(np.ascontiguousarray(xf)).to(DEV)
    di = torch.from_numpy(np.ascontiguousarray(xi)).to(DEV)
    tf = torch.tensor([df.data_ptr() + 4 * n_f * c for c in range(k)], dtype=torch.int64, device=DEV)
    ti = torch.tensor([di.data_ptr() + 8 * n_i * c for c in range(k)], dtype=torch.int64, device=DEV)
    # guard words behind both outputs: the kernel writes n elements and nothing else
    out_f = torch.full((n_f + 64,), -7.0, device=DEV)
    out_i = torch.full((n_i + 64,), -7.0, device=DEV)
    _lib.call("plato_agg_robust_columns", 0, tf.data_ptr(), ti.data_ptr() if n_i else None, k, 0, out_f.data_ptr(),
              out_i.data_ptr() if n_i else None, n_f, n_i, torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    assert bool((out_f[n_f:] == -7.0).all()) and bool((out_i[n_i:] == -7.0).all())
    return out_f[:n_f].cpu().numpy(), out_i[:n_i].cpu().numpy()


def assert_bits(got, exp):
    assert rc.canon(got).tobytes() == rc.canon(exp).tobytes()


@pytest.mark.parametrize("case", CASES, ids=[c["recipe"]["name"] for c in CASES])
def test_engine_median_equals_the_reference(engine, case, full):
    layout, xf, xi = rc.build_inputs(case["recipe"])
    payloads = rc.state_dicts(layout, xf, xi)
    got = engine.aggregate_robust(payloads, mode="median")
    assert list(got) == [e.name for e in layout.entries]
    got_f, got_i, dtypes = rc.flat_result(layout, got)
    assert dtypes == case["expected"]["dtypes"] == ["torch.float32"]  # the counters too
    for e in layout.entries:
        assert tuple(got[e.name].shape) == tuple(e.shape)
    check_against_fixture(case, got_f, got_i, xf, full)
    # on the mixed-zero columns the kernel's own rule holds: the total order -0 < +0
    exp_f, exp_i = ro.median(xf, xi)
    assert_bits(got_f, exp_f)
    assert_bits(got_i, exp_i)


@pytest.mark.parametrize("name", ["median_lenet5_k5", "median_resnet18_k8"])
def test_server_hook_median_equals_the_reference(name, full):
    case = next(c for c in CASES if c["recipe"]["name"] == name)
    layout, xf, xi = rc.build_inputs(case["recipe"])
    payloads = rc.state_dicts(layout, xf, xi)
    server = type("Server", (RobustAggregationMixin,), {"secure_aggregation_type": "Median",
                                                        "aggregation_device": "cuda:0"})()
    updates = [types.SimpleNamespace(report=types.SimpleNamespace(num_samples=10)) for _ in payloads]
    got = asyncio.run(server.aggregate_weights(updates, payloads[0], payloads))
    got_f, got_i, dtypes = rc.flat_result(layout, got)
    assert dtypes == ["torch.float32"]
    check_against_fixture(case, got_f, got_i, xf, full)
    items = server.get_logged_items()
    k = case["recipe"]["k"]
    assert server._plato_amd_timings["bytes"] == (k + 1) * layout.n_f32 * 4 + k * layout.n_i64 * 8 + layout.n_i64 * 4
    assert items["aggregation_kernel_ms"] > 0 and server._plato_amd_timings["robust_median_ms"] > 0


@pytest.mark.parametrize("k", KS)
def test_kernel_equals_the_restatement_on_random_layouts(k):
    rng = np.random.default_rng(1000 + k)
    for n_f in (1, 63, 64, 65, 1000, 4099):
        for n_i in (0, 1, 5):
            # few distinct values: ties across the median in most columns; both zero signs among them
            pool = np.concatenate([rng.standard_normal(6).astype(np.float32),
                                   np.array([0.0, -0.0, np.inf, -np.inf, 1e-42, -1e-42], dtype=np.float32)])
            xf = rng.standard_normal((k, n_f)).astype(np.float32)
            ties = rng.random((k, n_f)) < 0.5
            xf[ties] = pool[rng.integers(0, pool.size, int(ties.sum()))]
            xi = rng.integers(-(1 << 40), 1 << 40, (k, n_i), dtype=np.int64)
            got_f, got_i = device_median(xf, xi)
            exp_f, exp_i = ro.median(xf, xi)
            assert_bits(got_f, exp_f)
            assert_bits(got_i, exp_i)


@pytest.mark.parametrize("k", [1, 2, 5, 8, 33, 256])
def test_special_values(k):
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    cols = [np.full(k, nan, dtype=np.float32),                                  # K identical NaNs
            np.where(np.arange(k) == k // 2, nan, np.arange(k, dtype=np.float32)),  # one NaN among finite values
            np.resize(np.array([-inf, inf, inf, -inf, 0.0, 1.0], dtype=np.float32), k),  # -inf..+inf, duplicates
            np.full(k, 1.5, dtype=np.float32),                                  # all equal
            np.resize(np.array([1e-45, -1e-45, 3e-45], dtype=np.float32), k),   # subnormals
            np.resize(np.array([-0.0, 0.0], dtype=np.float32), k)]              # both zeros
    neg_nan = np.full(k, 1.0, dtype=np.float32)
    neg_nan.view(np.uint32)[0] = 0xFFC00001                                     # a negative NaN with a payload
    cols.append(neg_nan)
    xf = np.stack(cols, axis=1)
    xi = np.stack([np.resize(np.array([(1 << 24) + 1, -(1 << 24) - 1, (1 << 53) + 1], dtype=np.int64), k),
                   np.resize(np.array([-(1 << 24) - 1, -(1 << 24) - 3], dtype=np.int64), k)], axis=1)
    got_f, got_i = device_median(xf, xi)
    exp_f, exp_i = ro.median(xf, xi)
    assert_bits(got_f, exp_f)
    assert_bits(got_i, exp_i)
    assert np.isnan(got_f[0]) and np.isnan(got_f[1]) and np.isnan(got_f[6])
    assert got_f[3] == np.float32(1.5) and got_f[4] != 0  # no flush to zero
    # torch on the host agrees wherever it is defined bitwise (no NaN, no mixed zeros)
    ref = torch.median(torch.from_numpy(xf[:, 2:5].copy()), dim=0)[0].numpy()
    assert_bits(got_f[2:5], ref)
    ref_i = torch.median(torch.from_numpy(xi).to(torch.float32), dim=0)[0].numpy()
    assert_bits(got_i, ref_i)


def test_full_size_resnet18_k128_sampled():
    layout = ArenaLayout.from_shapes(workloads.resnet(18, 10))
    k, seed = 128, 23
    base = DeviceArena(layout, DEV)
    slab = ClientSlab(layout, k, DEV)
    fill_baseline(base, seed)
    fill_clients(slab, base, seed, k)
    pf, pi = slab.row_pointers(range(k))
    tf, ti = torch.from_numpy(pf).to(DEV), torch.from_numpy(pi).to(DEV)
    n_f, n_i = layout.n_f32, layout.n_i64
    out_f = torch.full((layout.row_f32,), float("nan"), device=DEV)
    out_i = torch.full((layout.row_i64,), float("nan"), device=DEV)
    _lib.call("plato_agg_robust_columns", 0, tf.data_ptr(), ti.data_ptr(), k, 0, out_f.data_ptr(), out_i.data_ptr(),
              n_f, n_i, torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    rng = np.random.default_rng(5)
    idx = np.unique(np.concatenate([rng.integers(0, n_f, 8192), [0, n_f - 1]]))
    idx_t = torch.from_numpy(idx).to(DEV)
    xf = slab.f32[:, :n_f].index_select(1, idx_t).cpu().numpy()
    xi = slab.i64[:, :n_i].cpu().numpy()
    exp_f, exp_i = ro.median(xf, xi)
    assert_bits(out_f[:n_f].index_select(0, idx_t).cpu().numpy(), exp_f)
    assert_bits(out_i[:n_i].cpu().numpy(), exp_i)
    assert not bool(torch.isnan(out_f[:n_f]).any())
    del slab, base
    torch.cuda.empty_cache()


def test_arrival_staged_rows_give_the_put_client_result(engine):
    case = next(c for c in CASES if c["recipe"]["name"] == "median_lenet5_k8")
    layout, xf, xi = rc.build_inputs(case["recipe"])
    payloads = rc.state_dicts(layout, xf, xi)
    staged = engine.aggregate_robust(payloads)
    eng = FedAvgEngine(DEV)
    try:
        for p in payloads:
            assert eng.prestage(p, ArenaLayout.from_state_dict(p))
        rnd = eng.begin(payloads[0], len(payloads))
        assert all(rnd.adopt(i, p) for i, p in enumerate(payloads))
        rnd.launch_robust("median")
        adopted = rnd.result()
    finally:
        eng.release_arrivals()
    for name in staged:
        assert adopted[name].dtype == torch.float32
        assert_bits(adopted[name].numpy().reshape(-1), staged[name].numpy().reshape(-1))


def test_delta_rounds_and_coded_payloads_are_refused():
    case = next(c for c in CASES if c["recipe"]["name"] == "median_lenet5_k3")
    layout, xf, xi = rc.build_inputs(case["recipe"])
    payloads = rc.state_dicts(layout, xf, xi)
    eng = FedAvgEngine(DEV)
    eng.delta_arenas = True
    rnd = eng.begin(payloads[0], len(payloads))
    rnd.put_baseline(payloads[0])
    for i, p in enumerate(payloads):
        rnd.put_client(i, p)
    with pytest.raises(ValueError, match="holds deltas"):
        rnd.launch_robust("median")
    bf16 = [type(p)((n, t.to(torch.bfloat16)) for n, t in p.items()) for p in payloads]
    with pytest.raises(ValueError, match="native payloads"):
        FedAvgEngine(DEV).aggregate_robust(bf16)
    with pytest.raises(ValueError, match="unknown robust aggregation mode"):
        FedAvgEngine(DEV).aggregate_robust(payloads, mode="krum")
