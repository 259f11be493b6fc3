"""Sub-model aggregation on the GPU: plato_agg_submodel_mean through FedAvgEngine.aggregate_submodels and
the hook, against the numpy restatement (tests/submodel_oracle.py) and the reference fixtures
(tests/golden/submodel_*), bit for bit (NaNs canonicalised: the sign of inf - inf differs by machine).

Shape of the kernel (plato_amd/csrc/submodel.hip) that the sizes below walk around: a workgroup of 256 lanes
owns one tile of PLATO_AGG_SUBMODEL_TILE = 1,024 consecutive output elements of one entry, a lane four
elements 256 apart; client rows are packed back to back, so a box starts at any 4-byte offset.
"""

import asyncio
import types
from collections import OrderedDict

import numpy as np
import pytest
import torch

from plato_amd import _lib
from plato_amd import submodel as sm
from plato_amd.engine import FedAvgEngine
from plato_amd.servers import SubmodelAggregationMixin
from tests import submodel_cases as sc
from tests import submodel_oracle as so
from tests.test_submodel import NAMES, case_of, check_against_fixture, inputs, restated, same_bits

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TILE = _lib.PLATO_AGG_SUBMODEL_TILE
SENTINEL = -7.0


@pytest.fixture(scope="module")
def engine():
    return FedAvgEngine(DEV)


def on_device(engine, g, clients, rule):
    got = engine.aggregate_submodels(sc.as_torch(g), [sc.as_torch(c) for c in clients], rule)
    return OrderedDict((k, v.numpy()) for k, v in got.items())


def check(engine, g, clients, rule):
    """The device's result equals the restatement's bit for bit; returns (result, counts)."""
    want, counts = so.aggregate(g, clients, rule)
    got = on_device(engine, g, clients, rule)
    assert list(got) == list(want)
    for k in want:
        assert same_bits(got[k], want[k]), (k, np.flatnonzero(
            sc.canon(got[k]).reshape(-1).view(np.uint32) != sc.canon(want[k]).reshape(-1).view(np.uint32))[:8])
    return got, counts


def model(spec, seed, who=0):
    """name -> seeded ndarray for [(name, shape)] (all float32)."""
    return sc.fill([(n, s, sc.F32) for n, s in spec], seed, who)


def toy(rates, seed=7):
    g = sc.fill(sc.toy_spec(1.0), seed, 0)
    return g, [sc.fill(sc.toy_spec(r), seed, 1 + k) for k, r in enumerate(rates)]


# ------------------------------------------------------------------ the reference fixtures
@pytest.mark.parametrize("name", NAMES)
def test_fixture_cases_through_the_engine(engine, name):
    g, clients = inputs(name)
    got = on_device(engine, g, clients, case_of(name)["recipe"]["rule"])
    check_against_fixture(name, got)
    want = restated(name)[0]
    for k in want:
        assert same_bits(got[k], want[k]), k
        if not so.participates(k):  # a clone of the global model's entry, dtype kept
            assert got[k].dtype == g[k].dtype and got[k].tobytes() == g[k].tobytes()


# ------------------------------------------------------------------ odd extents, client counts
@pytest.mark.parametrize("rule", ["heterofl", "fedrolex"])
@pytest.mark.parametrize("rates", [(0.5,), (0.25, 1.0), (0.5, 0.125, 1.0, 0.25, 0.5)], ids=["K1", "K2", "K5"])
def test_toy_layout_with_odd_extents(engine, rule, rates):
    # 7 -> 4 -> 2 -> 1 channels and a 13-wide layer: client rows of 27-float runs, boxes at odd offsets
    g, clients = toy(rates)
    _, counts = check(engine, g, clients, rule)
    assert not counts["s_bias"].any()  # an entry that no client covers
    assert bool(counts["pos_weight"].any()) == (rule == "fedrolex")


def test_full_width_clients(engine):
    for k in (1, 3):
        g, clients = toy((1.0,) * k, seed=11)
        _, counts = check(engine, g, clients, "fedrolex")
        assert all((c == k).all() for n, c in counts.items() if n != "s_bias")


def test_257_clients(engine):
    rates = [(1.0, 0.5, 0.25, 0.125)[k % 4] for k in range(257)]
    g, clients = toy(rates, seed=13)
    _, counts = check(engine, g, clients, "fedrolex")
    assert counts["stem.weight"].max() == 257 and counts["stem.weight"].min() == 65


def test_a_client_with_a_zero_extent(engine):
    g, clients = toy((0.5, 0.25, 0.5), seed=17)
    clients[1]["stem.weight"] = np.zeros((0, 3, 3, 3), dtype=np.float32)
    clients[1]["head.weight"] = np.zeros((10, 0), dtype=np.float32)
    clients[2]["mix.bias"] = np.zeros((0,), dtype=np.float32)
    _, counts = check(engine, g, clients, "heterofl")
    assert counts["stem.weight"].max() == 2 and counts["head.weight"].max() == 2 and counts["mix.bias"].max() == 2


# ------------------------------------------------------------------ order
def test_the_order_of_the_clients_is_the_order_of_the_sum(engine):
    g = model([("a.weight", (4, 6))], 19)
    g["a.weight"][...] = 0.25
    xs = []
    for k, v in enumerate((1e8, 1.0, -1e8)):
        x = model([("a.weight", (3, 5))], 19, 1 + k)
        x["a.weight"][:2, :3] = v
        xs.append(x)
    fwd, _ = check(engine, g, xs, "heterofl")
    rev, _ = check(engine, g, [xs[0], xs[2], xs[1]], "heterofl")
    assert fwd["a.weight"][0, 0] == np.float32(-0.25) / np.float32(3)  # 1 is lost against 1e8 + 0.25
    assert rev["a.weight"][0, 0] == np.float32(0.75) / np.float32(3)   # ((0.25 + 1e8) - 1e8 + 1) - 0.25
    assert not same_bits(fwd["a.weight"], rev["a.weight"])


# ------------------------------------------------------------------ special values
def test_special_values(engine):
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    g = model([("a.weight", (4, 8)), ("b.bias", (8,))], 23)
    xs = [model([("a.weight", (2, 4)), ("b.bias", (4,))], 23, 1 + k) for k in range(3)]
    a = g["a.weight"]
    a[0, 0], a[0, 1], a[0, 2], a[0, 3] = inf, -inf, nan, -0.0        # covered
    a[3, 4], a[3, 5], a[3, 6], a[3, 7] = inf, -inf, nan, -0.0        # uncovered
    a[1, 0], a[1, 1] = 1e8, 0.0
    for x in xs:
        x["a.weight"][1, 1] = np.float32(3e-45)                      # subnormal sums: 3 * 2 * 2^-149
    xs[1]["a.weight"][1, 2] = nan                                    # a client's NaN stays in its element
    xs[2]["b.bias"][3] = inf
    got, counts = check(engine, g, xs, "heterofl")
    out = got["a.weight"]
    assert np.isnan(out[0, :3]).all() and np.isnan(out[3, 4:7]).all()
    assert out[3, 7].tobytes() == np.float32(0.0).tobytes()          # (-0 - -0) / 1 = +0
    assert out[0, 3] != 0 and np.isfinite(out[0, 3])                 # -0 + x
    assert out[1, 0] == 0.0                                          # the clients' low bits are lost against 1e8
    assert out[1, 1] == np.float32(3e-45) and 0 < out[1, 1] < 1e-44  # (2 + 2 + 2) * 2^-149 / 3
    assert np.isnan(out[1, 2]) and np.isnan(out).sum() == 7
    assert got["b.bias"][3] == inf and np.isfinite(np.delete(got["b.bias"], 3)).all()
    assert not out[2].any() and not out[:3, 4:].any()                # uncovered finite elements are +0


# ------------------------------------------------------------------ tile boundaries
@pytest.mark.parametrize("s1", [1, 2049, 5000])
def test_rows_that_cross_tiles(engine, s1):
    # the 3-float entry in front puts the next entry's output at an offset that is not 16-byte aligned
    g = model([("z.bias", (3,)), ("a.weight", (3, 5000)), ("c.weight", (4099, 1, 1, 1))], 29)
    xs = [model([("z.bias", (z,)), ("a.weight", (r, c)), ("c.weight", (m, 1, 1, 1))], 29, 1 + k)
          for k, (z, r, c, m) in enumerate(((3, 3, s1, 4099), (1, 2, 5000, 1025), (2, 1, 1023, 0)))]
    assert sm.global_layout(sc.as_torch(g))["a.weight"].offset % 4 == 3
    _, counts = check(engine, g, xs, "heterofl")
    assert counts["a.weight"][0].min() >= 1 and counts["c.weight"].reshape(-1)[1025] == 1


def test_direct_call_writes_its_entries_and_nothing_else():
    """Two entries with a gap between them, the output prefilled: the gap and the guard stay untouched."""
    rng = np.random.default_rng(31)
    n_out, k = 2 * TILE + 77, 3
    gflat = rng.standard_normal(n_out).astype(np.float32)
    entries = np.array([[5, 3, 1, 341, 0, 0], [TILE + 30, 2, 3, 173, 1, 0]], dtype=np.int64)  # 1023 and 1038 elements
    boxes = np.array([[[3, 1, 341, 2], [2, 1, 100, 0], [0, 0, 0, -1]],
                      [[2, 3, 173, 1025], [1, 2, 7, 200], [2, 1, 173, 1]]], dtype=np.int64)
    row_len = np.array([1025 + 1038, 214, 347], dtype=np.int64)
    rows = [rng.standard_normal(int(n)).astype(np.float32) for n in row_len]
    want = np.full(n_out, SENTINEL, dtype=np.float32)
    for e, (off, P, Q, L, _, _) in enumerate(entries):
        gv = gflat[off:off + P * Q * L].reshape(P, Q, L)
        acc, cnt = gv.copy(), np.zeros((P, Q, L), dtype=np.int32)
        for c in range(k):
            p, q, l, src = boxes[e, c]
            if src >= 0:
                acc[:p, :q, :l] = acc[:p, :q, :l] + rows[c][src:src + p * q * l].reshape(p, q, l)
                cnt[:p, :q, :l] += 1
        want[off:off + P * Q * L] = ((acc - gv) / np.maximum(cnt, 1).astype(np.float32)).reshape(-1)
    d_g = torch.from_numpy(gflat).to(DEV)
    d_rows = [torch.from_numpy(r).to(DEV) for r in rows]
    table = torch.tensor([r.data_ptr() for r in d_rows], dtype=torch.int64, device=DEV)
    out = torch.full((n_out + 64,), SENTINEL, dtype=torch.float32, device=DEV)
    nbytes = _lib.lib().plato_agg_submodel_tables_bytes(k, len(entries))
    work = torch.full((nbytes + 256,), 0x5A, dtype=torch.uint8, device=DEV)
    _lib.call("plato_agg_submodel_mean", d_g.data_ptr(), table.data_ptr(), k, row_len.ctypes.data, entries.ctypes.data,
              boxes.ctypes.data, len(entries), work.data_ptr(), out.data_ptr(), n_out,
              torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got[:n_out].tobytes() == want.tobytes()
    assert (got[n_out:] == SENTINEL).all() and bool((work[nbytes:] == 0x5A).all())


# ------------------------------------------------------------------ reuse across calls
def test_calls_with_other_signatures_and_after_an_ordinary_round(engine):
    g, clients = toy((0.5, 0.25), seed=37)
    first, _ = check(engine, g, clients, "fedrolex")
    g2, clients2 = toy((0.125, 1.0, 0.5), seed=41)
    check(engine, g2, clients2, "heterofl")
    again, _ = check(engine, g, clients, "fedrolex")  # the cached layouts and stagers of the first call
    assert all(same_bits(first[k], again[k]) for k in first)
    # an ordinary FedAvg round on the same engine in between
    base = sc.as_torch(sc.fill(sc.toy_spec(1.0), 43, 0))
    payloads = [sc.as_torch(sc.fill(sc.toy_spec(1.0), 43, 1 + i)) for i in range(2)]
    fed = engine.aggregate_weights(base, payloads, [0.25, 0.75])
    want = base["head.bias"] + ((payloads[0]["head.bias"] - base["head.bias"]) * 0.25
                                + (payloads[1]["head.bias"] - base["head.bias"]) * 0.75)
    assert torch.allclose(fed["head.bias"], want, rtol=1e-5, atol=1e-7)  # (its own tests pin its bits)
    check(engine, g2, clients2, "fedrolex")
    check(engine, *inputs("resnet18_small_partial"), "fedrolex")


# ------------------------------------------------------------------ the hook
def test_hook_on_a_real_engine(engine):
    g, clients = toy((0.5, 1.0, 0.25), seed=47)
    server = type("Server", (SubmodelAggregationMixin,), {"submodel_rule": "fedrolex"})()
    server._plato_amd_engine = engine
    gt = sc.as_torch(g)
    server.algorithm = types.SimpleNamespace(model=types.SimpleNamespace(state_dict=lambda: gt))
    stale = OrderedDict((k, torch.full_like(v, 9)) for k, v in gt.items())  # baseline_weights is not read
    got = asyncio.run(server.aggregate_weights([], stale, [sc.as_torch(c) for c in clients]))
    want = so.aggregate(g, clients, "fedrolex")[0]
    assert all(same_bits(got[k].numpy(), want[k]) for k in want)
    assert got["norm.num_batches_tracked"].dtype == torch.int64
    t = server._plato_amd_timings
    assert t["submodel_mean_ms"] > 0 and t["kernel_ms"] == t["submodel_mean_ms"]
    assert t["bytes"] == sm.build_tables(
        sm.global_layout(gt), [sm.client_signature(sm.global_layout(gt), "fedrolex", sc.as_torch(c), "c")
                               for c in clients], "fedrolex").algorithmic_bytes()
