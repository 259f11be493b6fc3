"""Elastic sub-model aggregation on the GPU: plato_agg_elastic_mean through FedAvgEngine.aggregate_elastic and the
hook, against the numpy restatement (tests/elastic_oracle.py) and the reference fixtures (tests/golden/elastic_*),
bit for bit (NaNs canonicalised: the sign of inf - inf differs by machine).

Shape of the kernel (plato_amd/csrc/elastic.hip) that the sizes below walk around: a workgroup of 256 lanes
owns one tile of PLATO_AGG_ELASTIC_TILE = 1,024 consecutive output elements of one entry, a lane four elements
256 apart; an entry's view keeps as many extents as its holders cut, and a tile loops over the entry's own
boxes; client rows are packed back to back, so a box starts at any 4-byte offset.
"""

import asyncio
import types
from collections import OrderedDict

import numpy as np
import pytest
import torch

from plato_amd import _lib
from plato_amd import elastic as el
from plato_amd.engine import FedAvgEngine
from plato_amd.servers import ElasticAggregationMixin
from tests import elastic_cases as ec
from tests import elastic_oracle as eo
from tests import submodel_cases as sc
from tests.test_elastic import NAMES, case_of, check_against_fixture, inputs, restated, same_bits

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TILE = _lib.PLATO_AGG_ELASTIC_TILE
SENTINEL = -7.0


@pytest.fixture(scope="module")
def engine():
    return FedAvgEngine(DEV)


def on_device(engine, g, clients, update_track=True):
    got = engine.aggregate_elastic(ec.as_torch(g), [ec.as_torch(c) for c in clients], update_track)
    assert all(v.dtype == torch.float32 for v in got.values())
    return OrderedDict((k, v.numpy().copy()) for k, v in got.items())


def check(engine, g, clients, update_track=True):
    """The device's result equals the restatement's bit for bit; returns (result, counts)."""
    want, counts = eo.aggregate(g, clients, update_track)
    got = on_device(engine, g, clients, update_track)
    assert list(got) == list(want)
    for k in want:
        assert same_bits(got[k], want[k]), (k, np.flatnonzero(
            ec.canon(got[k]).reshape(-1).view(np.uint32) != ec.canon(want[k]).reshape(-1).view(np.uint32))[:8])
    return got, counts


def model(spec, seed, who=0):
    """name -> seeded ndarray for [(name, shape)] (all float32)."""
    return sc.fill([(n, s, sc.F32) for n, s in spec], seed, who)


def toy(configs, seed=7):
    g = sc.fill(ec.toy_spec(ec.TOY_GLOBAL), seed, 0)
    return g, [sc.fill(ec.toy_spec(c), seed, 1 + k) for k, c in enumerate(configs)]


# ------------------------------------------------------------------ the reference fixtures
@pytest.mark.parametrize("name", NAMES)
def test_fixture_cases_through_the_engine(engine, name):
    g, clients = inputs(name)
    got = on_device(engine, g, clients, case_of(name)["recipe"]["update_track"])
    check_against_fixture(name, got)
    want = restated(name)[0]
    for k in want:
        assert same_bits(got[k], want[k]), k


# ------------------------------------------------------------------ boxes on four dims
BOXES = [(2, 5, 7, 11), (3, 4, 7, 11), (3, 5, 6, 11), (3, 5, 7, 10), (1, 1, 1, 1)]


@pytest.mark.parametrize("which", [None, 0, 1, 2, 3, 4], ids=["K5", "a", "b", "c", "d", "one"])
def test_an_entry_cut_on_each_of_its_four_dims(engine, which):
    # 1,155 elements: the second tile holds the last 131; alone, a client that is full in its trailing dims
    # merges them (one division per element, or none), together they keep all four extents (three divisions)
    g = model([("a.weight", (3, 5, 7, 11))], 53)
    xs = [model([("a.weight", s)], 53, 1 + k) for k, s in enumerate(BOXES)]
    xs = xs if which is None else [xs[which]]
    tab = el.ElasticRound(object(), ec.as_torch(g), [ec.as_torch(x) for x in xs]).tables
    view = tuple(int(v) for v in tab.entries[0, 1:5])
    assert view == {None: (3, 5, 7, 11), 0: (1, 1, 1, 1155), 1: (1, 1, 3, 385), 2: (1, 3, 5, 77), 3: (3, 5, 7, 11),
                    4: (3, 5, 7, 11)}[which]
    _, counts = check(engine, g, xs)
    c = counts["a.weight"]
    assert c[0, 0, 0, 0] == len(xs) and c.max() == len(xs) and c[2, 4, 6, 10] == 0


# ------------------------------------------------------------------ client counts, missing keys, empty rows
@pytest.mark.parametrize("k", [1, 2, 257])
def test_toy_layout_by_client_count(engine, k):
    g, clients = toy([ec.TOY_CLIENTS[i % 3] for i in range(k)])
    _, counts = check(engine, g, clients)
    assert not counts["pos"].any() and not counts["scale"].any()  # rank 0: nobody takes part
    assert counts["conv.weight"].max() == k and counts["conv.weight"][6, 2, 4, 4] == 0
    assert counts["extra.weight"].max() == k // 3  # only every third client holds it: nobody for K < 3
    assert counts["mix.weight"].min() == (k + 1) // 3


def test_an_entry_without_a_box_and_clients_without_a_row(engine):
    g, clients = toy(ec.TOY_CLIENTS[:2], seed=11)
    tab = el.ElasticRound(object(), ec.as_torch(g), [ec.as_torch(c) for c in clients]).tables
    names = [e.name for e in el.global_layout(ec.as_torch(g))[0].entries]
    assert [n for n, e in zip(names, tab.entries) if e[7] == 0] == ["pos", "scale", "extra.weight", "extra.bias"]
    got, _ = check(engine, g, clients)
    assert not got["extra.weight"].any() and not got["norm.num_batches_tracked"].any()
    # clients that hold nothing, first, in the middle and last; one that holds rank-0 keys and strangers only
    empty, strangers = OrderedDict(), OrderedDict(pos=clients[0]["pos"], other=np.ones(5, dtype=np.float32))
    first, counts = check(engine, g, [empty, clients[0], strangers, clients[1], empty])
    assert counts["conv.bias"].max() == 2 and all(same_bits(first[k], got[k]) for k in got)
    only, counts = check(engine, g, [empty, strangers])  # every row is empty: all (g - g) / 1
    assert not any(c.any() for c in counts.values()) and not any(v.any() for v in only.values())


def test_a_client_with_a_zero_extent(engine):
    g, clients = toy(ec.TOY_CLIENTS, seed=17)
    clients[0]["conv.weight"] = np.zeros((4, 0, 3, 3), dtype=np.float32)
    clients[1]["mix.weight"] = np.zeros((0, 7, 3, 3), dtype=np.float32)
    clients[1]["head.weight"] = np.zeros((10, 0), dtype=np.float32)
    clients[2]["conv.bias"] = np.zeros((0,), dtype=np.float32)
    _, counts = check(engine, g, clients)
    assert all(counts[k].max() == 2 for k in ("conv.weight", "mix.weight", "head.weight", "conv.bias"))


# ------------------------------------------------------------------ order
def test_the_order_of_the_clients_is_the_order_of_the_sum(engine):
    g = model([("a.weight", (4, 6, 2, 2)), ("b.running_mean", (5,))], 19)
    g["a.weight"][...] = 1e8
    a, b = model([("a.weight", (3, 5, 2, 1))], 19, 1), model([("a.weight", (2, 6, 1, 2)), ("b.running_mean", (5,))], 19, 2)
    a["a.weight"][...], b["a.weight"][...] = 6.0, -4.0
    fwd, _ = check(engine, g, [a, b])
    rev, _ = check(engine, g, [b, a])
    # against 1e8 (spacing 8): 6 rounds up to 8, then -4 ties back to the even 1e8; -4 first ties to 1e8, then 6 adds 8
    assert fwd["a.weight"][0, 0, 0, 0] == 0.0 and rev["a.weight"][0, 0, 0, 0] == 4.0
    assert fwd["a.weight"][2, 0, 0, 0] == 8.0 and fwd["a.weight"][0, 5, 0, 0] == 0.0  # one client each: 8 / 1, 0 / 1
    assert not same_bits(fwd["a.weight"], rev["a.weight"])
    assert same_bits(fwd["b.running_mean"], rev["b.running_mean"])


# ------------------------------------------------------------------ special values
def test_special_values(engine):
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    g = model([("a.weight", (4, 8, 1, 2)), ("b.bias", (8,)), ("c.weight", (3, 3))], 23)
    xs = [model([("a.weight", (2, 4, 1, 1)), ("b.bias", (4,))], 23, 1 + k) for k in range(3)]
    a = g["a.weight"]
    a[0, 0, 0, 0], a[0, 1, 0, 0], a[0, 2, 0, 0], a[0, 3, 0, 0] = inf, -inf, nan, -0.0   # covered
    a[3, 4, 0, 1], a[3, 5, 0, 1], a[3, 6, 0, 1], a[3, 7, 0, 1] = inf, -inf, nan, -0.0   # uncovered
    g["c.weight"][0] = inf, nan, -0.0                                                   # held by nobody
    a[1, 0, 0, 0], a[1, 1, 0, 0] = 1e8, 0.0
    for x in xs:
        x["a.weight"][1, 1, 0, 0] = np.float32(3e-45)                # subnormal sums: 3 * 2 * 2^-149
    xs[1]["a.weight"][1, 2, 0, 0] = nan                              # a client's NaN stays in its element
    xs[2]["b.bias"][3] = inf
    got, counts = check(engine, g, xs)
    out = got["a.weight"]
    assert np.isnan(out[0, :3, 0, 0]).all() and np.isnan(out[3, 4:7, 0, 1]).all()
    assert out[3, 7, 0, 1].tobytes() == np.float32(0.0).tobytes()    # (-0 - -0) / 1 = +0
    assert out[0, 3, 0, 0] != 0 and np.isfinite(out[0, 3, 0, 0])     # -0 + x
    assert out[1, 0, 0, 0] == 0.0                                    # the clients' low bits are lost against 1e8
    assert out[1, 1, 0, 0] == np.float32(3e-45) and 0 < out[1, 1, 0, 0] < 1e-44  # (2 + 2 + 2) * 2^-149 / 3
    assert np.isnan(out[1, 2, 0, 0]) and np.isnan(out).sum() == 7
    assert got["b.bias"][3] == inf and np.isfinite(np.delete(got["b.bias"], 3)).all()
    assert not out[2].any() and not out[:, :, :, 1][~np.isnan(out[:, :, :, 1])].any()  # uncovered finite elements: +0
    c = got["c.weight"]
    assert np.isnan(c[0, :2]).all() and c[0, 2].tobytes() == np.float32(0.0).tobytes() and not c[1:].any()


# ------------------------------------------------------------------ tile boundaries
@pytest.mark.parametrize("s1", [1, 2049, 5000])
def test_rows_that_cross_tiles(engine, s1):
    # the 3-float entry in front puts the next entry's output at an offset that is not 16-byte aligned
    g = model([("z.bias", (3,)), ("a.weight", (3, 5000)), ("c.weight", (4099, 1, 1, 1)), ("d.weight", (70, 5, 3, 3))], 29)
    xs = [model([("z.bias", (z,)), ("a.weight", (r, c)), ("c.weight", (m, 1, 1, 1)), ("d.weight", d)], 29, 1 + k)
          for k, (z, r, c, m, d) in enumerate(((3, 3, s1, 4099, (70, 5, 3, 3)), (1, 2, 5000, 1025, (33, 5, 3, 2)),
                                               (2, 1, 1023, 0, (70, 2, 1, 3))))]
    del xs[2]["z.bias"]
    assert el.global_layout(ec.as_torch(g))[0]["a.weight"].offset % 4 == 3
    _, counts = check(engine, g, xs)
    assert counts["a.weight"][0].min() >= 1 and counts["c.weight"].reshape(-1)[1025] == 1
    assert counts["d.weight"][69, 4, 2, 2] == 1 and counts["d.weight"][0, 0, 0, 0] == 3  # 3,150 elements, four tiles


def test_direct_call_writes_its_entries_and_nothing_else():
    """Three entries with gaps between them, the output prefilled: the gaps and the guard stay untouched."""
    rng = np.random.default_rng(31)
    n_out, k = 2 * TILE + 77, 4
    gflat = rng.standard_normal(n_out).astype(np.float32)
    # 1,023 elements at 5; 1,038 at 1,054 (two tiles); 20 at 2,100 that nobody holds
    entries = np.array([[5, 3, 1, 11, 31, 0, 0, 2], [TILE + 30, 2, 3, 1, 173, 1, 2, 3], [2100, 1, 1, 1, 20, 3, 5, 0]],
                       dtype=np.int64)
    boxes = np.array([[3, 1, 11, 31, 2, 0], [2, 1, 5, 7, 0, 2],
                      [2, 3, 1, 173, 1025, 0], [1, 2, 1, 7, 200, 1], [2, 1, 1, 173, 70, 2]], dtype=np.int64)
    row_len = np.array([1025 + 1038, 214, 416, 0], dtype=np.int64)  # client 3 holds nothing
    rows = [rng.standard_normal(int(n)).astype(np.float32) for n in row_len]
    want = np.full(n_out, SENTINEL, dtype=np.float32)
    for off, A, B, C, D, _, first, n in entries:
        gv = gflat[off:off + A * B * C * D].reshape(A, B, C, D)
        acc, cnt = gv.copy(), np.zeros(gv.shape, dtype=np.int32)
        for a, b, c, d, src, client in boxes[first:first + n]:
            acc[:a, :b, :c, :d] = acc[:a, :b, :c, :d] + rows[client][src:src + a * b * c * d].reshape(a, b, c, d)
            cnt[:a, :b, :c, :d] += 1
        want[off:off + gv.size] = ((acc - gv) / np.maximum(cnt, 1).astype(np.float32)).reshape(-1)
    d_g = torch.from_numpy(gflat).to(DEV)
    d_rows = [torch.from_numpy(r if r.size else np.zeros(1, dtype=np.float32)).to(DEV) for r in rows]
    table = torch.tensor([r.data_ptr() for r in d_rows], dtype=torch.int64, device=DEV)
    out = torch.full((n_out + 64,), SENTINEL, dtype=torch.float32, device=DEV)
    nbytes = _lib.lib().plato_agg_elastic_tables_bytes(len(entries), len(boxes))
    work = torch.full((nbytes + 256,), 0x5A, dtype=torch.uint8, device=DEV)
    _lib.call("plato_agg_elastic_mean", d_g.data_ptr(), table.data_ptr(), k, row_len.ctypes.data, entries.ctypes.data,
              len(entries), boxes.ctypes.data, len(boxes), work.data_ptr(), out.data_ptr(), n_out,
              torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got[:n_out].tobytes() == want.tobytes()
    assert (want[:5] == SENTINEL).all() and (want[2120:] == SENTINEL).all() and (want[2092:2100] == SENTINEL).all()
    assert (got[n_out:] == SENTINEL).all() and bool((work[nbytes:] == 0x5A).all())


# ------------------------------------------------------------------ reuse across calls
def test_calls_with_other_signatures_and_after_an_ordinary_round(engine):
    g, clients = toy(ec.TOY_CLIENTS[:2], seed=37)
    first, _ = check(engine, g, clients)
    g2, clients2 = toy(ec.TOY_CLIENTS[::-1], seed=41)
    check(engine, g2, clients2, update_track=False)
    again, _ = check(engine, g, clients)  # the cached layouts and stagers of the first call
    assert all(same_bits(first[k], again[k]) for k in first)
    # an ordinary FedAvg round on the same engine in between
    base = sc.as_torch(sc.fill(sc.toy_spec(1.0), 43, 0))
    payloads = [sc.as_torch(sc.fill(sc.toy_spec(1.0), 43, 1 + i)) for i in range(2)]
    fed = engine.aggregate_weights(base, payloads, [0.25, 0.75])
    want = base["head.bias"] + ((payloads[0]["head.bias"] - base["head.bias"]) * 0.25
                                + (payloads[1]["head.bias"] - base["head.bias"]) * 0.75)
    assert torch.allclose(fed["head.bias"], want, rtol=1e-5, atol=1e-7)  # (its own tests pin its bits)
    check(engine, g2, clients2)
    check(engine, *inputs("resnet_small_partial"))
    # and a width-only round of the other sub-model path, which keeps a slab of its own
    gs, cs = sc.build(SUBMODEL["toy_heterofl"])
    engine.aggregate_submodels(sc.as_torch(gs), [sc.as_torch(c) for c in cs], "heterofl")
    again, _ = check(engine, g, clients)
    assert all(same_bits(first[k], again[k]) for k in first)


# ------------------------------------------------------------------ against the width-only kernel
SUBMODEL = {r["name"]: r for r in sc.recipes()}


@pytest.mark.parametrize("name", ["resnet18_small", "resnet18_small_special", "toy_heterofl"])
def test_width_only_inputs_equal_the_width_only_kernel(engine, name):
    """Clients that hold every key and cut the first two dims only: the float32 weight / bias entries (ranks 1,
    2 and 4, and the toy's 3-D and 0-D entries that nobody covers under either rule) come out of
    plato_agg_elastic_mean as they come out of plato_agg_submodel_mean.  The keys that pass through there (running
    statistics, counters) are averaged or zeroed here by contract and are not compared."""
    g, clients = sc.build(SUBMODEL[name])
    gt, payloads = sc.as_torch(g), [sc.as_torch(c) for c in clients]
    old = engine.aggregate_submodels(gt, payloads, "heterofl")
    new = engine.aggregate_elastic(gt, payloads)
    compared = [k for k, v in g.items() if v.dtype == np.float32 and ("weight" in k or "bias" in k)]
    assert {g[k].ndim for k in compared} >= {1, 2, 4}
    for k in compared:
        assert same_bits(new[k].numpy(), old[k].numpy()), k


# ------------------------------------------------------------------ the hook
def test_hook_on_a_real_engine(engine):
    g, clients = toy(ec.TOY_CLIENTS, seed=47)
    server = type("Server", (ElasticAggregationMixin,), {})()
    server._plato_amd_engine = engine
    gt = ec.as_torch(g)
    server.algorithm = types.SimpleNamespace(model=types.SimpleNamespace(state_dict=lambda: gt))
    stale = OrderedDict((k, torch.full_like(v, 9)) for k, v in gt.items())  # baseline_weights is not read
    got = asyncio.run(server.aggregate_weights([], stale, [ec.as_torch(c) for c in clients]))
    want = eo.aggregate(g, clients)[0]
    assert list(got) == list(want) and all(same_bits(got[k].numpy(), want[k]) for k in want)
    assert got["norm.num_batches_tracked"].dtype == torch.float32
    t = server._plato_amd_timings
    assert t["elastic_mean_ms"] > 0 and t["kernel_ms"] == t["elastic_mean_ms"]
    glayout = el.global_layout(gt)[0]
    assert t["bytes"] == el.build_tables(
        glayout, [el.client_signature(glayout, ec.as_torch(c), True, "c") for c in clients]).algorithmic_bytes()
    assert t["bytes"] == 4 * (2 * 1212 + 276 + 480 + 235)
