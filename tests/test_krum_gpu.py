"""Multi-Krum on the GPU: plato_agg_pairwise_sqdist and plato_agg_mean_rows against the numpy restatements
(tests/krum_oracle.py), and the engine and hook against the reference fixtures (tests/golden/krum_*).

Tiling of the distance kernel (plato_amd/csrc/krum.hip) that the shapes below walk around: 8 x 8 client
blocks per wave, 32 x 32 client tiles per workgroup, 128-coordinate LDS panels, fp32 chains of
PLATO_AGG_PAIRDIST_CHAIN terms per lane (64 * CHAIN = 8,192 coordinates), coordinate chunks of 8,192
coordinates for models this small (one workgroup each).  The client counts and the coordinate counts
are independent grid dimensions of the kernel: every coordinate count is run at every K up to 33 (one
and three tiles, every block count), the four large K (three to 36 tiles) at the coordinate counts up to
two chunks, which keeps the float64 restatement of a case within a second or two.
"""

import asyncio
import types

import numpy as np
import pytest
import torch

from plato_amd import _lib, workloads
from plato_amd.arena import ArenaLayout
from plato_amd.engine import ClientSlab, DeviceArena, FedAvgEngine
from plato_amd.krum import multi_krum_select
from plato_amd.multi import MultiDeviceEngine
from plato_amd.servers import RobustAggregationMixin
from plato_amd.synthetic import fill_baseline, fill_clients
from tests import krum_cases as kc
from tests import krum_oracle as ko
from tests.test_krum import check_mean_against_fixture

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CASES = kc.load_cases()
LENET = [c for c in CASES if c["recipe"]["model"] == "lenet5"]
CHAIN = _lib.PLATO_AGG_PAIRDIST_CHAIN
CHUNK = 64 * CHAIN  # coordinates per chunk (and per chain) at these sizes
KS_SMALL = (1, 2, 3, 7, 8, 9, 31, 32, 33)       # +-1 around the 8-client block and the 32-client tile
KS_LARGE = (64, 65, 255, 256)
NS = (1, 63, 64, 65, 127, 128, 129, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1)
NS_LARGE_K = (1, 63, 64, 65, 257, CHUNK + 1)
NIS = (0, 1, 3)
SENTINEL = -7.0


@pytest.fixture(scope="module")
def engine():
    return FedAvgEngine(DEV)


@pytest.fixture(scope="module")
def full():
    return kc.load_full()


def tolerance(d: int) -> float:
    """Relative: the fp32 chains ((CHAIN + 1) * 2^-24) and the float64 sums of both sides (D * 2^-53)."""
    return (CHAIN + 1) * 2.0 ** -24 + d * 2.0 ** -53


def tables(xf: np.ndarray, xi: np.ndarray, order=None):
    k, n_f, n_i = xf.shape[0], xf.shape[1], xi.shape[1]
    order = range(k) if order is None else order
    df = torch.from_numpy(np.ascontiguousarray(xf)).to(DEV)
    di = torch.from_numpy(np.ascontiguousarray(xi)).to(DEV)
    tf = torch.tensor([df.data_ptr() + 4 * n_f * c for c in order], dtype=torch.int64, device=DEV)
    ti = torch.tensor([di.data_ptr() + 8 * n_i * c for c in order], dtype=torch.int64, device=DEV)
    return (df, di), tf, ti


def device_sqdist(xf: np.ndarray, xi: np.ndarray, order=None) -> np.ndarray:
    """plato_agg_pairwise_sqdist on [K, n] host matrices; the output is sentinel-filled and 64 guard
    elements follow the output and the workspace: the kernels write their own elements and nothing else."""
    keep, tf, ti = tables(xf, xi, order)
    got = launch_sqdist(tf, ti, xf.shape[1], xi.shape[1])
    del keep
    return got


def launch_sqdist(tf: torch.Tensor, ti: torch.Tensor, n_f: int, n_i: int) -> np.ndarray:
    """device_sqdist on pointer tables that are on the device already, with the same guards."""
    k = tf.numel()
    nbytes = _lib.lib().plato_agg_pairwise_sqdist_workspace(k, n_f, n_i)
    assert nbytes >= 256 and nbytes % 256 == 0
    work = torch.full((nbytes // 8 + 64,), SENTINEL, dtype=torch.float64, device=DEV)
    out = torch.full((k * k + 64,), SENTINEL, dtype=torch.float64, device=DEV)
    _lib.call("plato_agg_pairwise_sqdist", tf.data_ptr() if n_f else None, ti.data_ptr() if n_i else None, k, n_f, n_i,
              work.data_ptr(), out.data_ptr(), torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    assert bool((out[k * k:] == SENTINEL).all()) and bool((work[nbytes // 8:] == SENTINEL).all())
    return out[: k * k].cpu().numpy().reshape(k, k)


def device_mean(xf: np.ndarray, xi: np.ndarray, order):
    n_f, n_i = xf.shape[1], xi.shape[1]
    keep, tf, ti = tables(xf, xi, order)
    out_f = torch.full((n_f + 64,), SENTINEL, device=DEV)
    out_i = torch.full((n_i + 64,), SENTINEL, device=DEV)
    _lib.call("plato_agg_mean_rows", tf.data_ptr() if n_f else None, ti.data_ptr() if n_i else None, len(order),
              out_f.data_ptr() if n_f else None, out_i.data_ptr() if n_i else None, n_f, n_i,
              torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    assert bool((out_f[n_f:] == SENTINEL).all()) and bool((out_i[n_i:] == SENTINEL).all())
    del keep
    return out_f[:n_f].cpu().numpy(), out_i[:n_i].cpu().numpy()


def clients(rng, k: int, n_f: int, n_i: int):
    """A common model plus small noise (the shape that a Gram-form distance would cancel), counters nearby."""
    base = rng.standard_normal(n_f).astype(np.float32)
    xf = (base + np.float32(2.0 ** -7) * rng.standard_normal((k, n_f)).astype(np.float32)).astype(np.float32)
    xi = rng.integers(0, 10001, n_i, dtype=np.int64) + rng.integers(0, 9, (k, n_i), dtype=np.int64)
    return xf, xi


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def assert_matrix(got: np.ndarray, exp: np.ndarray, d: int):
    k = got.shape[0]
    assert np.array_equal(np.isnan(got), np.isnan(exp))
    ok = ~np.isnan(exp)
    with np.errstate(invalid="ignore"):
        err, lim = np.abs(got[ok] - exp[ok]), tolerance(d) * np.abs(exp[ok])
    fin = np.isfinite(exp[ok])
    assert np.all(err[fin] <= lim[fin]), float(np.max(err[fin] / np.maximum(np.abs(exp[ok][fin]), 1e-300)))
    assert np.array_equal(got[ok][~fin], exp[ok][~fin])  # +inf stays +inf
    assert not bits(np.diagonal(got)).any()  # exactly +0
    assert np.array_equal(bits(got), bits(got.T.copy()))  # symmetric bitwise
    assert got.shape == (k, k)


@pytest.mark.parametrize("k", KS_SMALL + KS_LARGE)
def test_distances_equal_the_restatement(k):
    rng = np.random.default_rng(2000 + k)
    for at, n_f in enumerate(NS if k in KS_SMALL else NS_LARGE_K):
        for n_i in (NIS if k in KS_SMALL else (NIS[at % 3],)):
            xf, xi = clients(rng, k, n_f, n_i)
            assert_matrix(device_sqdist(xf, xi), ko.pairwise_sqdist(xf, xi), n_f + n_i)


def test_counters_above_2_to_24_round_to_even():
    xi = np.array([[(1 << 24) + 1], [(1 << 24) + 3], [0], [-(1 << 24) - 1]], dtype=np.int64)
    for xf in (np.zeros((4, 0), dtype=np.float32), np.zeros((4, 5), dtype=np.float32)):
        got = device_sqdist(xf, xi)
        assert got[0, 1] == 16.0  # 2^24 and 2^24 + 4; 4.0 without the rounding
        assert got[0, 2] == 2.0 ** 48 and got[0, 3] == 2.0 ** 50 and got[2, 3] == 2.0 ** 48  # exact squares
        assert_matrix(got, ko.pairwise_sqdist(xf, xi), xf.shape[1] + 1)


def test_nan_and_infinities_propagate_by_ieee_rules():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    xf = np.array([[1.0, nan, 2.0], [inf, 0.5, 2.0], [inf, 0.25, 1.0], [-inf, 0.0, 0.0], [3.0, 1.0, 0.0],
                   [3.0, 1.0, 0.0]], dtype=np.float32)
    got = device_sqdist(xf, np.zeros((6, 0), dtype=np.int64))
    assert np.isnan(got[0, 1:]).all() and np.isnan(got[1:, 0]).all()  # a NaN client
    assert np.isnan(got[1, 2])                                        # inf - inf
    assert got[1, 3] == np.inf and got[1, 4] == np.inf and got[3, 4] == np.inf
    assert got[4, 5] == 0.0 and not bits(got[4:, 4:]).any()           # identical clients: exactly +0
    assert not bits(np.diagonal(got)).any()                          # the diagonal: +0 for the NaN and inf rows too
    assert_matrix(got, ko.pairwise_sqdist(xf, np.zeros((6, 0), dtype=np.int64)), 3)


def test_matrix_is_repeatable_and_independent_of_table_order_and_of_k():
    rng = np.random.default_rng(77)
    k, n_f, n_i = 65, 2 * CHUNK + 77, 3
    xf, xi = clients(rng, k, n_f, n_i)
    first = device_sqdist(xf, xi)
    assert np.array_equal(bits(first), bits(device_sqdist(xf, xi)))  # two runs
    perm = rng.permutation(k)
    assert perm.tolist() != list(range(k))
    assert np.array_equal(bits(device_sqdist(xf, xi, perm)), bits(first[np.ix_(perm, perm)]))
    sub = [64, 3, 40, 7, 33, 12, 0, 31, 32]  # K = 9: other tiles, other blocks, the same pairs
    assert np.array_equal(bits(device_sqdist(xf, xi, sub)), bits(first[np.ix_(sub, sub)]))
    assert_matrix(first, ko.pairwise_sqdist(xf, xi), n_f + n_i)


def canon(a):
    return kc.canon(a)


@pytest.mark.parametrize("m", [1, 2, 3, 250])
def test_mean_rows_equals_the_sequential_restatement_bit_for_bit(m):
    rng = np.random.default_rng(3000 + m)
    k = m + 3
    for n in (1, 63, 65):
        xf = rng.standard_normal((k, n)).astype(np.float32)
        xi = rng.integers(-(1 << 40), 1 << 40, (k, n), dtype=np.int64)
        xf[:, 0] = -0.0                      # every row -0: +0 + -0 = +0, then +0 / m
        xi[rng.integers(0, k), 0] = (1 << 24) + 1
        if n > 1:
            xf[rng.integers(0, k), 1] = np.nan
            xf[:, 2] = np.float32(1e-42)     # subnormals: no flush to zero
            xf[0, 3], xf[1 % k, 3] = np.inf, -np.inf
        order = rng.permutation(k)[:m].tolist()
        got_f, got_i = device_mean(xf, xi, order)
        exp_f, exp_i = ko.mean_rows(xf, xi, order)
        assert np.array_equal(bits(canon(got_f)), bits(canon(exp_f)))
        assert np.array_equal(bits(canon(got_i)), bits(canon(exp_i)))
        assert not bits(got_f[:1]).any()
        if n > 1:
            assert got_f[2] != 0


@pytest.mark.parametrize("case", LENET, ids=[c["recipe"]["name"] for c in LENET])
def test_engine_multi_krum_equals_the_reference(engine, case, full):
    recipe = case["recipe"]
    layout, xf, xi = kc.build_inputs(recipe)
    payloads = kc.state_dicts(layout, xf, xi)
    got = engine.aggregate_multi_krum(payloads, f=recipe["f"])
    assert engine.last_selected == case["expected"]["selection"]  # exactly and in order
    assert list(got) == [e.name for e in layout.entries]
    got_f, got_i, dtypes = kc.flat_result(layout, got)
    assert dtypes == case["expected"]["dtypes"] == ["torch.float32"]
    for e in layout.entries:
        assert tuple(got[e.name].shape) == tuple(e.shape)
    check_mean_against_fixture(case, got_f, got_i, xf, xi, full)
    exp_dist = ko.pairwise_sqdist(xf, xi)
    sel = ko.select(exp_dist, recipe["f"])
    exp_f, exp_i = ko.mean_rows(xf, xi, sel)
    assert sel == engine.last_selected
    assert np.array_equal(bits(got_f), bits(exp_f)) and np.array_equal(bits(got_i), bits(exp_i))
    # the round API: the matrix in its own right, then the launch
    rnd = engine.begin(payloads[0], len(payloads))
    rnd.deltas = False
    for i, p in enumerate(payloads):
        rnd.put_client(i, p)
    dist = rnd.launch_pairwise_sqdist()
    assert dist.dtype == np.float64 and dist.shape == (recipe["k"], recipe["k"])
    assert_matrix(dist, exp_dist, layout.n_f32 + layout.n_i64)
    assert rnd.timings["pairwise_sqdist_ms"] > 0
    rnd.launch_multi_krum(recipe["f"])
    again = rnd.result()
    assert rnd.selected == case["expected"]["selection"]
    for name in got:
        assert np.array_equal(bits(again[name].numpy().reshape(-1)), bits(got[name].numpy().reshape(-1)))
    t = rnd.timings
    assert t["pairwise_sqdist_ms"] > 0 and t["mean_rows_ms"] > 0 and t["select_ms"] > 0 and t["kernel_ms"] > 0


def test_resnet18_fixture_and_server_hook(full):
    """The hook on the ResNet-18 fixture (int64 counters among the entries) and on a lenet5 one."""
    for name in ("mkrum_resnet18_k8", "mkrum_lenet5_k16"):
        case = next(c for c in CASES if c["recipe"]["name"] == name)
        layout, xf, xi = kc.build_inputs(case["recipe"])
        payloads = kc.state_dicts(layout, xf, xi)
        server = type("Server", (RobustAggregationMixin,), {"secure_aggregation_type": "Multi-krum",
                                                            "aggregation_device": "cuda:0"})()
        updates = [types.SimpleNamespace(report=types.SimpleNamespace(num_samples=10)) for _ in payloads]
        got = asyncio.run(server.aggregate_weights(updates, payloads[0], payloads))
        got_f, got_i, dtypes = kc.flat_result(layout, got)
        assert dtypes == ["torch.float32"]
        check_mean_against_fixture(case, got_f, got_i, xf, xi, full)
        exp_f, exp_i = ko.mean_rows(xf, xi, case["expected"]["selection"])
        assert np.array_equal(bits(got_f), bits(exp_f)) and np.array_equal(bits(got_i), bits(exp_i))
        t = server._plato_amd_timings
        assert t["pairwise_sqdist_ms"] > 0 and t["mean_rows_ms"] > 0 and server.get_logged_items()["aggregation_kernel_ms"] > 0


def test_arrival_staged_rows_give_the_put_client_result(engine):
    case = next(c for c in CASES if c["recipe"]["name"] == "mkrum_lenet5_k9")
    layout, xf, xi = kc.build_inputs(case["recipe"])
    payloads = kc.state_dicts(layout, xf, xi)
    staged = engine.aggregate_multi_krum(payloads)
    eng = FedAvgEngine(DEV)
    try:
        for p in payloads:
            assert eng.prestage(p, ArenaLayout.from_state_dict(p))
        rnd = eng.begin(payloads[0], len(payloads))
        assert all(rnd.adopt(i, p) for i, p in enumerate(payloads))
        rnd.launch_multi_krum(2)
        adopted = rnd.result()
    finally:
        eng.release_arrivals()
    assert rnd.selected == case["expected"]["selection"]
    for name in staged:
        assert adopted[name].dtype == torch.float32
        assert np.array_equal(bits(adopted[name].numpy().reshape(-1)), bits(staged[name].numpy().reshape(-1)))


def test_delta_rounds_coded_payloads_small_k_and_several_gpus_are_refused():
    case = next(c for c in CASES if c["recipe"]["name"] == "mkrum_lenet5_k7")
    layout, xf, xi = kc.build_inputs(case["recipe"])
    payloads = kc.state_dicts(layout, xf, xi)
    eng = FedAvgEngine(DEV)
    eng.delta_arenas = True
    rnd = eng.begin(payloads[0], len(payloads))
    rnd.put_baseline(payloads[0])
    for i, p in enumerate(payloads):
        rnd.put_client(i, p)
    with pytest.raises(ValueError, match="holds deltas"):
        rnd.launch_multi_krum(2)
    with pytest.raises(ValueError, match="holds deltas"):
        rnd.launch_pairwise_sqdist()
    bf16 = [type(p)((n, t.to(torch.bfloat16)) for n, t in p.items()) for p in payloads]
    with pytest.raises(ValueError, match="native payloads"):
        FedAvgEngine(DEV).aggregate_multi_krum(bf16)
    with pytest.raises(ValueError, match="more than 6 clients, got 6"):
        FedAvgEngine(DEV).aggregate_multi_krum(payloads[:6])
    eng6 = FedAvgEngine(DEV)
    rnd = eng6.begin(payloads[0], 6)
    rnd.deltas = False
    for i, p in enumerate(payloads[:6]):
        rnd.put_client(i, p)
    with pytest.raises(ValueError, match="more than 6 clients, got 6"):
        rnd.launch_multi_krum(2)
    with pytest.raises(NotImplementedError, match="one GPU"):
        MultiDeviceEngine(["cuda:0", "cuda:0"]).aggregate_multi_krum(payloads)


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
    nbytes = _lib.lib().plato_agg_pairwise_sqdist_workspace(k, n_f, n_i)
    work = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    out = torch.full((k, k), float("nan"), dtype=torch.float64, device=DEV)
    _lib.call("plato_agg_pairwise_sqdist", tf.data_ptr(), ti.data_ptr(), k, n_f, n_i, work.data_ptr(), out.data_ptr(),
              torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    dist = out.cpu().numpy()
    assert not np.isnan(dist).any() and not bits(np.diagonal(dist)).any()
    assert np.array_equal(bits(dist), bits(dist.T.copy()))
    rng = np.random.default_rng(5)
    pairs = {(0, 1), (0, 127), (31, 32), (63, 64), (126, 127)}  # first, last, across tile borders
    while len(pairs) < 16:
        i, j = (int(v) for v in rng.integers(0, k, 2))
        if i != j:
            pairs.add((i, j))
    rows = {}
    for i in sorted({c for p in pairs for c in p}):
        rows[i] = np.concatenate([slab.f32[i, :n_f].cpu().numpy(), slab.i64[i, :n_i].cpu().numpy().astype(np.float32)])
    for i, j in sorted(pairs):
        d = (rows[i] - rows[j]).astype(np.float64)
        exp = float(np.dot(d, d))
        assert abs(dist[i, j] - exp) <= tolerance(n_f + n_i) * exp, (i, j)
    sel = multi_krum_select(dist, 2)
    assert len(sel) == len(set(sel)) == 122 and all(0 <= s < k for s in sel)
    del slab, base, work, out
    torch.cuda.empty_cache()
