"""Bulyan and Trimmed-mean on the GPU: the nearest-mean mode of plato_agg_robust_columns against the numpy
restatement (tests/nearest_oracle.py), bit for bit, and the engine and the hook against the reference
fixtures (tests/golden/bulyan_*).

The kernel (plato_amd/csrc/robust.hip) has one coordinate per lane and one-wave workgroups, so the
coordinate counts walk around 64; every loop over the K rows is unrolled by 8, so the client counts walk
around 8 and its multiples, up to the 256 that fill the 64 KiB of LDS.
"""

import asyncio
import types

import numpy as np
import pytest
import torch

from plato_amd import _lib, workloads
from plato_amd.arena import ArenaLayout
from plato_amd.engine import ClientSlab, DeviceArena, FedAvgEngine
from plato_amd.krum import bulyan_select
from plato_amd.multi import MultiDeviceEngine
from plato_amd.servers import DetectorAggregationMixin
from plato_amd.synthetic import fill_baseline, fill_clients
from tests import bulyan_cases as bc
from tests import nearest_oracle as no
from tests.test_bulyan import check_values_against_fixture

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CASES = bc.load_cases()
LENET = [c for c in CASES if c["recipe"]["model"] == "lenet5"]
KS = (1, 2, 3, 4, 5, 8, 9, 33, 64, 65, 128, 255, 256)
SENTINEL = -7.0
MODE = _lib.PLATO_AGG_ROBUST["nearest_mean"]


@pytest.fixture(scope="module")
def engine():
    return FedAvgEngine(DEV)


@pytest.fixture(scope="module")
def full():
    return bc.load_full()


def trims(k: int):
    return sorted({t for t in (0, 1, (k - 1) // 2) if 0 <= 2 * t < k})


def tables(xf: np.ndarray, xi: np.ndarray, order=None):
    k, n_f, n_i = xf.shape[0], xf.shape[1], xi.shape[1]
    order = range(k) if order is None else order
    df = torch.from_numpy(np.ascontiguousarray(xf)).to(DEV)
    di = torch.from_numpy(np.ascontiguousarray(xi)).to(DEV)
    tf = torch.tensor([df.data_ptr() + 4 * n_f * c for c in order], dtype=torch.int64, device=DEV)
    ti = torch.tensor([di.data_ptr() + 8 * n_i * c for c in order], dtype=torch.int64, device=DEV)
    return (df, di), tf, ti


def device_nearest(xf: np.ndarray, xi: np.ndarray, trim: int, order=None):
    """plato_agg_robust_columns, nearest-mean mode, on [K, n] host matrices."""
    keep, tf, ti = tables(xf, xi, order)
    n_f, n_i = xf.shape[1], xi.shape[1]
    k = tf.numel()
    out_f = torch.full((n_f + 64,), SENTINEL, device=DEV)
    out_i = torch.full((n_i + 64,), SENTINEL, device=DEV)
    _lib.call("plato_agg_robust_columns", MODE, tf.data_ptr() if n_f else None, ti.data_ptr() if n_i else None, k,
              trim, out_f.data_ptr() if n_f else None, out_i.data_ptr() if n_i else None, n_f, n_i,
              torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    assert bool((out_f[n_f:] == SENTINEL).all()) and bool((out_i[n_i:] == SENTINEL).all())
    del keep
    return out_f[:n_f].cpu().numpy(), out_i[:n_i].cpu().numpy()


def device_mean(xf: np.ndarray, xi: np.ndarray, order):
    keep, tf, ti = tables(xf, xi, order)
    n_f, n_i = xf.shape[1], xi.shape[1]
    out_f = torch.full((n_f + 64,), SENTINEL, device=DEV)
    out_i = torch.full((n_i + 64,), SENTINEL, device=DEV)
    _lib.call("plato_agg_mean_rows", tf.data_ptr() if n_f else None, ti.data_ptr() if n_i else None, len(order),
              out_f.data_ptr() if n_f else None, out_i.data_ptr() if n_i else None, n_f, n_i,
              torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    assert bool((out_f[n_f:] == SENTINEL).all()) and bool((out_i[n_i:] == SENTINEL).all())
    del keep
    return out_f[:n_f].cpu().numpy(), out_i[:n_i].cpu().numpy()


def assert_bits(got, exp):
    assert bc.canon(got).tobytes() == bc.canon(exp).tobytes()


# multiples of 1/4 around 1: m +- d pairs, so that two different values are equally far from many medians
GRID = np.array([1.0, 0.75, 1.25, 0.5, 1.5, 0.25, 1.75, 0.0, 2.0], dtype=np.float32)
POOL = np.concatenate([GRID, np.array([0.0, -0.0, np.inf, -np.inf, 1e-42, -1e-42], dtype=np.float32)])
POOL_I = np.array([100, 99, 101, 98, 102, 97, 103, (1 << 24) + 1, (1 << 24) + 3, -(1 << 24) - 1], dtype=np.int64)


def tied_columns(rng, k: int, n_f: int, n_i: int, pool=POOL):
    """Half of every column from a small pool of m +- d pairs: distance ties straddle the cut in most
    columns, and the table-order rule decides."""
    xf = (1.0 + 0.5 * rng.standard_normal((k, n_f))).astype(np.float32)
    ties = rng.random((k, n_f)) < 0.5
    xf[ties] = pool[rng.integers(0, pool.size, int(ties.sum()))]
    xi = rng.integers(-(1 << 40), 1 << 40, (k, n_i), dtype=np.int64)
    ties = rng.random((k, n_i)) < 0.5
    xi[ties] = POOL_I[rng.integers(0, POOL_I.size, int(ties.sum()))]
    return xf, xi


@pytest.mark.parametrize("k", KS)
def test_kernel_equals_the_restatement_on_random_layouts(k):
    rng = np.random.default_rng(4000 + k)
    straddled = 0
    for n_f in (1, 63, 64, 65, 1000):
        for n_i in (0, 1, 5):
            xf, xi = tied_columns(rng, k, n_f, n_i)
            for trim in trims(k):
                got_f, got_i = device_nearest(xf, xi, trim)
                exp_f, exp_i = no.nearest_mean(xf, xi, trim)
                assert_bits(got_f, exp_f)
                assert_bits(got_i, exp_i)
                straddled += no.boundary_tie_columns(xf, trim).size
    assert straddled > 0 or k < 4  # the tie rule was exercised (K >= 4: a trim that drops rows exists)


@pytest.mark.parametrize("k", [1, 2, 5, 8, 33, 256])
def test_special_values(k):
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    cols = [np.full(k, nan, dtype=np.float32),                                  # 0: K identical NaNs
            np.where(np.arange(k) == k // 2, nan, np.arange(k, dtype=np.float32)),  # 1: one NaN among finite values
            np.resize(np.array([inf, inf, 1.0, inf, -inf, 2.0], dtype=np.float32), k),  # 2: median +inf, equal infs
            np.resize(np.array([-inf, -inf, 1.0, -inf, inf, -inf], dtype=np.float32), k),  # 3: median -inf
            np.full(k, 1.5, dtype=np.float32),                                  # 4: all equal
            np.resize(np.array([-0.0, 0.0], dtype=np.float32), k),              # 5: both zeros
            np.resize(np.array([1e-45, 3e-45, 7e-45], dtype=np.float32), k)]     # 6: subnormals
    neg_nan = np.full(k, 1.0, dtype=np.float32)
    neg_nan.view(np.uint32)[0] = 0xFFC00001                                     # 7: a negative NaN with a payload
    cols.append(neg_nan)
    xf = np.stack(cols, axis=1)
    xi = np.stack([np.resize(np.array([(1 << 24) + 1, -(1 << 24) - 1, (1 << 53) + 1], dtype=np.int64), k),
                   np.resize(np.array([-(1 << 24) - 1, -(1 << 24) - 3, -(1 << 24) - 5], dtype=np.int64), k)], axis=1)
    for trim in trims(k):
        got_f, got_i = device_nearest(xf, xi, trim)
        exp_f, exp_i = no.nearest_mean(xf, xi, trim)
        assert_bits(got_f, exp_f)
        assert_bits(got_i, exp_i)
        assert [int(v) for v in got_f.view(np.uint32)[[0, 1, 7]]] == [0x7FC00000] * 3  # the canonical NaN itself
        assert got_f[4] == np.float32(1.5) and got_f[5] == 0 and not np.signbit(got_f[5])  # +0 + -0 = +0
        assert got_f[6] != 0  # no flush to zero
        if 2 * trim == k - 1:  # b = 1: the lower median itself (finite: its own distance is 0)
            med_i = np.sort(xi.astype(np.float32), axis=0)[(k - 1) // 2]
            assert_bits(got_i, med_i)
    if k >= 5:  # the NaN distances of the equal infinities rank after the +inf distances of the finite values
        keys = no.distance_keys(xf[:, 2:3])[:, 0]
        assert set(keys.tolist()) == {0x7FC00000, 0x7F800000}


@pytest.mark.parametrize("k", [1, 5, 64, 256])
def test_trim_0_equals_mean_rows_bit_for_bit_on_the_same_table(k):
    rng = np.random.default_rng(5000 + k)
    xf, xi = tied_columns(rng, k + 2, 1000, 5)
    xf[0, :3] = (np.nan, np.inf, -np.inf)
    order = rng.permutation(k + 2)[:k].tolist()
    got_f, got_i = device_nearest(xf, xi, 0, order)
    mean_f, mean_i = device_mean(xf, xi, order)
    assert_bits(got_f, mean_f)
    assert_bits(got_i, mean_i)


def test_permuted_table_changes_ties_and_summation_order_only():
    rng = np.random.default_rng(78)
    k, trim, n_f, n_i = 33, 5, 1000, 5
    xf, xi = tied_columns(rng, k, n_f, n_i, pool=GRID)  # finite values: the bound below is finite
    first = device_nearest(xf, xi, trim)
    again = device_nearest(xf, xi, trim)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()  # two runs
    perm = rng.permutation(k)
    assert perm.tolist() != list(range(k))
    got = device_nearest(xf, xi, trim, perm)
    exp = no.nearest_mean(xf[perm], xi[perm], trim)
    assert_bits(got[0], exp[0])
    assert_bits(got[1], exp[1])
    for x, a, b in ((xf, first[0], got[0]), (xi, first[1], got[1])):
        tie = np.zeros(x.shape[1], dtype=bool)
        tie[no.boundary_tie_columns(x, trim)] = True
        assert np.array_equal(np.flatnonzero(tie), no.boundary_tie_columns(x[perm], trim))  # a property of the column
        # no boundary tie: the same kept values, summed in another order
        err = np.abs(a.astype(np.float64) - b.astype(np.float64))
        assert np.all(err[~tie] <= no.value_bound(x, trim)[~tie] + 2 * 2.0 ** -24 * np.abs(a[~tie]))
    assert no.boundary_tie_columns(xf, trim).size > 0 and (first[0] != got[0]).any()


def _payload_case(name):
    case = next(c for c in CASES if c["recipe"]["name"] == name)
    layout, xf, xi = bc.build_inputs(case["recipe"])
    return case, layout, xf, xi, bc.state_dicts(layout, xf, xi)


def _check_result(case, layout, got, xf, xi, full, sel):
    """Dtypes, shapes, the reference within the bound off the listed columns, the restatement bit for bit."""
    assert list(got) == [e.name for e in layout.entries]
    got_f, got_i, dtypes = bc.flat_result(layout, got)
    assert dtypes == case["expected"]["dtypes"] == ["torch.float32"]  # the counters too
    for e in layout.entries:
        assert tuple(got[e.name].shape) == tuple(e.shape)
    check_values_against_fixture(case, got_f, got_i, xf, xi, full)
    trim = bc.trim_of(case["recipe"])
    if case["recipe"]["model"] == "lenet5":
        exp_f, exp_i = no.nearest_mean(xf[sel], xi[sel], trim)
        assert_bits(got_f, exp_f)
        assert_bits(got_i, exp_i)
    else:  # full size: 8,192 sampled coordinates and every counter
        idx = np.unique(np.concatenate([np.random.default_rng(6).integers(0, layout.n_f32, 8192), [0, layout.n_f32 - 1]]))
        assert_bits(got_f[idx], no.nearest_mean_columns(xf[sel][:, idx], trim))
        assert_bits(got_i, no.nearest_mean_columns(xi[sel], trim))


@pytest.mark.parametrize("case", CASES, ids=[c["recipe"]["name"] for c in CASES])
def test_engine_equals_the_reference_and_the_restatement(engine, case, full):
    recipe = case["recipe"]
    layout, xf, xi = bc.build_inputs(recipe)
    payloads = bc.state_dicts(layout, xf, xi)
    rnd = engine.begin(payloads[0], len(payloads))
    rnd.deltas = False
    for i, p in enumerate(payloads):
        rnd.put_client(i, p)
    if recipe["kind"] == "Bulyan":
        got = engine.aggregate_bulyan(payloads, f=recipe["f"])
        assert engine.last_selected == case["expected"]["selection"]  # exactly and in order
        sel = engine.last_selected
        rnd.launch_bulyan(recipe["f"])
    else:
        got = engine.aggregate_robust(payloads, mode="nearest_mean")
        sel = list(range(recipe["k"]))
        rnd.launch_robust("nearest_mean", 0)
    _check_result(case, layout, got, xf, xi, full, sel)
    again = rnd.result()  # the round API
    for name in got:
        assert again[name].numpy().tobytes() == got[name].numpy().tobytes()
    t = rnd.timings
    assert t["robust_nearest_mean_ms"] > 0 and t["kernel_ms"] > 0
    if recipe["kind"] == "Bulyan":
        assert rnd.selected == case["expected"]["selection"]
        assert t["pairwise_sqdist_ms"] > 0 and t["select_ms"] > 0


def test_engine_nearest_mean_with_a_trim(engine):
    case, layout, xf, xi, payloads = _payload_case("trimmed_lenet5_k33")
    got = engine.aggregate_robust(payloads, mode="nearest_mean", trim=7)
    got_f, got_i, dtypes = bc.flat_result(layout, got)
    exp_f, exp_i = no.nearest_mean(xf, xi, 7)
    assert dtypes == ["torch.float32"]
    assert_bits(got_f, exp_f)
    assert_bits(got_i, exp_i)
    with pytest.raises(ValueError, match="trim"):
        engine.aggregate_robust(payloads, mode="nearest_mean", trim=17)


@pytest.mark.parametrize("name", ["bulyan_resnet18_k6_f1", "bulyan_lenet5_k16_f3", "trimmed_resnet18_k8",
                                  "trimmed_lenet5_k8"])
def test_detector_hook_equals_the_reference(name, full):
    case, layout, xf, xi, payloads = _payload_case(name)
    recipe = case["recipe"]
    server = type("Server", (DetectorAggregationMixin,), {"secure_aggregation_type": recipe["kind"],
                                                          "num_attackers": recipe["f"],
                                                          "aggregation_device": "cuda:0"})()
    updates = [types.SimpleNamespace(report=types.SimpleNamespace(num_samples=10)) for _ in payloads]
    got = asyncio.run(server.aggregate_weights(updates, payloads[0], payloads))
    sel = case["expected"]["selection"] if recipe["kind"] == "Bulyan" else list(range(recipe["k"]))
    _check_result(case, layout, got, xf, xi, full, sel)
    t = server._plato_amd_timings
    assert t["robust_nearest_mean_ms"] > 0 and server.get_logged_items()["aggregation_kernel_ms"] > 0
    if recipe["kind"] == "Bulyan":
        assert t["pairwise_sqdist_ms"] > 0 and t["select_ms"] > 0


# Bulyan on ResNet-18 (int64 counters among the entries) at the issue's (K, f) = (13, 3), for which no
# reference fixture can be generated (tests/bulyan_cases.py): against the restatement.  Seed 10010 has the
# widest score gap found, 0.049 relative, four orders above what the device distances may differ by.
RESNET_13_3 = {"model": "resnet18", "k": 13, "seed": 10010, "f": 3}


@pytest.fixture(scope="module")
def resnet_13_3():
    """(layout, payloads, restated selection, sampled fp32 coordinates, their restated values, the restated
    counters), computed once."""
    layout, xf, xi = bc.build_inputs(RESNET_13_3)
    k, f = RESNET_13_3["k"], RESNET_13_3["f"]
    cols = np.concatenate([xf, xi.astype(np.float32)], axis=1)
    dist = np.zeros((k, k))
    for i in range(k):  # krum_oracle.pairwise_sqdist's arithmetic, one pass per pair
        for j in range(i + 1, k):
            d = (cols[i] - cols[j]).astype(np.float64)
            dist[i, j] = dist[j, i] = float(np.dot(d, d))
    sel = no.bulyan_select(dist, f)
    assert len(sel) == 7 and sel != list(range(7))
    idx = np.unique(np.concatenate([np.random.default_rng(7).integers(0, layout.n_f32, 8192), [0, layout.n_f32 - 1]]))
    exp_f = no.nearest_mean_columns(xf[sel][:, idx], f)
    exp_i = no.nearest_mean_columns(xi[sel], f)
    assert layout.n_i64 > 0 and np.unique(exp_i).size > 1  # counters that differ: a wrong table would show
    return layout, bc.state_dicts(layout, xf, xi), sel, idx, exp_f, exp_i


def _check_resnet_13_3(resnet_13_3, got, selected):
    layout, _, sel, idx, exp_f, exp_i = resnet_13_3
    assert selected == sel  # exactly and in order
    assert list(got) == [e.name for e in layout.entries]
    got_f, got_i, dtypes = bc.flat_result(layout, got)
    assert dtypes == ["torch.float32"]  # the counters too
    for e in layout.entries:
        assert tuple(got[e.name].shape) == tuple(e.shape)
    assert_bits(got_f[idx], exp_f)
    assert_bits(got_i, exp_i)
    assert got_i.size == layout.n_i64 and not np.isnan(got_f).any()


def test_engine_bulyan_on_resnet18_k13_f3_equals_the_restatement(engine, resnet_13_3):
    payloads = resnet_13_3[1]
    got = engine.aggregate_bulyan(payloads, RESNET_13_3["f"])
    _check_resnet_13_3(resnet_13_3, got, engine.last_selected)


def test_round_launch_bulyan_on_resnet18_k13_f3_equals_the_restatement(engine, resnet_13_3):
    payloads = resnet_13_3[1]
    rnd = engine.begin(payloads[0], len(payloads))
    rnd.deltas = False
    for i, p in enumerate(payloads):
        rnd.put_client(i, p)
    rnd.launch_bulyan(RESNET_13_3["f"])
    _check_resnet_13_3(resnet_13_3, rnd.result(), rnd.selected)
    t = rnd.timings
    assert t["pairwise_sqdist_ms"] > 0 and t["select_ms"] > 0 and t["robust_nearest_mean_ms"] > 0
    lay = resnet_13_3[0]
    assert rnd.algorithmic_bytes() == (13 + 7 + 1) * lay.n_f32 * 4 + (13 + 7) * lay.n_i64 * 8 + lay.n_i64 * 4


def test_detector_hook_bulyan_on_resnet18_k13_f3_equals_the_restatement(resnet_13_3):
    payloads = resnet_13_3[1]
    server = type("Server", (DetectorAggregationMixin,), {"secure_aggregation_type": "Bulyan",
                                                          "num_attackers": RESNET_13_3["f"],
                                                          "aggregation_device": "cuda:0"})()
    updates = [types.SimpleNamespace(report=types.SimpleNamespace(num_samples=10)) for _ in payloads]
    got = asyncio.run(server.aggregate_weights(updates, payloads[0], payloads))
    _check_resnet_13_3(resnet_13_3, got, server.aggregation_engine().last_selected)
    assert server._plato_amd_timings["robust_nearest_mean_ms"] > 0


def test_arrival_staged_rows_give_the_put_client_result(engine):
    case, layout, xf, xi, payloads = _payload_case("bulyan_lenet5_k9_f2")
    staged = engine.aggregate_bulyan(payloads, 2)
    staged_mean = engine.aggregate_robust(payloads, mode="nearest_mean", trim=1)
    eng = FedAvgEngine(DEV)
    try:
        for p in payloads:
            assert eng.prestage(p, ArenaLayout.from_state_dict(p))
        rnd = eng.begin(payloads[0], len(payloads))
        assert all(rnd.adopt(i, p) for i, p in enumerate(payloads))
        rnd.launch_bulyan(2)
        adopted = rnd.result()
        rnd.launch_robust("nearest_mean", 1)
        adopted_mean = rnd.result()
    finally:
        eng.release_arrivals()
    assert rnd.selected == case["expected"]["selection"]
    for a, b in ((adopted, staged), (adopted_mean, staged_mean)):
        for name in b:
            assert a[name].dtype == torch.float32
            assert_bits(a[name].numpy().reshape(-1), b[name].numpy().reshape(-1))


def test_delta_rounds_coded_payloads_small_k_and_several_gpus_are_refused():
    case, layout, xf, xi, payloads = _payload_case("bulyan_lenet5_k6_f1")
    eng = FedAvgEngine(DEV)
    eng.delta_arenas = True
    rnd = eng.begin(payloads[0], len(payloads))
    rnd.put_baseline(payloads[0])
    for i, p in enumerate(payloads):
        rnd.put_client(i, p)
    with pytest.raises(ValueError, match="holds deltas"):
        rnd.launch_bulyan(1)
    with pytest.raises(ValueError, match="holds deltas"):
        rnd.launch_robust("nearest_mean", 1)
    bf16 = [type(p)((n, t.to(torch.bfloat16)) for n, t in p.items()) for p in payloads]
    with pytest.raises(ValueError, match="native payloads"):
        FedAvgEngine(DEV).aggregate_bulyan(bf16, 1)
    with pytest.raises(ValueError, match="native payloads"):
        FedAvgEngine(DEV).aggregate_robust(bf16, mode="nearest_mean")
    with pytest.raises(ValueError, match="at least 6 clients, got 5"):
        FedAvgEngine(DEV).aggregate_bulyan(payloads[:5], 1)
    with pytest.raises(ValueError, match="at least 9 clients, got 6"):
        FedAvgEngine(DEV).aggregate_bulyan(payloads, 2)
    eng5 = FedAvgEngine(DEV)
    rnd = eng5.begin(payloads[0], 5)
    rnd.deltas = False
    for i, p in enumerate(payloads[:5]):
        rnd.put_client(i, p)
    with pytest.raises(ValueError, match="at least 6 clients, got 5"):
        rnd.launch_bulyan(1)
    with pytest.raises(NotImplementedError, match="one GPU"):
        MultiDeviceEngine(["cuda:0", "cuda:0"]).aggregate_bulyan(payloads, 1)
    with pytest.raises(NotImplementedError, match="one GPU"):
        MultiDeviceEngine(["cuda:0", "cuda:0"]).aggregate_robust(payloads, mode="nearest_mean")


def test_full_size_resnet18_k128_sampled():
    layout = ArenaLayout.from_shapes(workloads.resnet(18, 10))
    k, seed, f = 128, 23, 3
    base = DeviceArena(layout, DEV)
    slab = ClientSlab(layout, k, DEV)
    fill_baseline(base, seed)
    fill_clients(slab, base, seed, k)
    pf, pi = slab.row_pointers(range(k))
    tf, ti = torch.from_numpy(pf).to(DEV), torch.from_numpy(pi).to(DEV)
    n_f, n_i = layout.n_f32, layout.n_i64
    stream = torch.cuda.current_stream(DEV).cuda_stream
    nbytes = _lib.lib().plato_agg_pairwise_sqdist_workspace(k, n_f, n_i)
    work = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    dist_d = torch.full((k, k), float("nan"), dtype=torch.float64, device=DEV)
    _lib.call("plato_agg_pairwise_sqdist", tf.data_ptr(), ti.data_ptr(), k, n_f, n_i, work.data_ptr(),
              dist_d.data_ptr(), stream)
    sel = bulyan_select(dist_d.cpu().numpy(), f)
    assert len(sel) == len(set(sel)) == 122 and all(0 <= s < k for s in sel)
    sf, si = torch.from_numpy(pf[sel]).to(DEV), torch.from_numpy(pi[sel]).to(DEV)
    out_f = torch.full((layout.row_f32,), float("nan"), device=DEV)
    out_i = torch.full((layout.row_i64,), float("nan"), device=DEV)
    _lib.call("plato_agg_robust_columns", MODE, sf.data_ptr(), si.data_ptr(), len(sel), f, out_f.data_ptr(),
              out_i.data_ptr(), n_f, n_i, stream)
    torch.cuda.synchronize()
    rng = np.random.default_rng(5)
    idx = np.unique(np.concatenate([rng.integers(0, n_f, 8192), [0, n_f - 1]]))
    idx_t = torch.from_numpy(idx).to(DEV)
    sel_t = torch.tensor(sel, device=DEV)
    xf = slab.f32[:, :n_f].index_select(1, idx_t).index_select(0, sel_t).cpu().numpy()
    xi = slab.i64[:, :n_i].index_select(0, sel_t).cpu().numpy()
    exp_f, exp_i = no.nearest_mean(xf, xi, f)
    assert_bits(out_f[:n_f].index_select(0, idx_t).cpu().numpy(), exp_f)
    assert_bits(out_i[:n_i].cpu().numpy(), exp_i)
    assert not bool(torch.isnan(out_f[:n_f]).any())
    del slab, base, work, dist_d
    torch.cuda.empty_cache()
