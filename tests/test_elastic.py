"""Elastic sub-model aggregation without a GPU: the numpy restatement (tests/elastic_oracle.py) against the
reference fixtures (tests/golden/elastic_*) bit for bit, ranks and the table builder (plato_amd.elastic),
every refusal of plato_agg_elastic_mean and of the Python layer, and the hook on a stub engine."""

import asyncio
import functools
import os
import types
from collections import OrderedDict

import numpy as np
import pytest
import torch

from plato_amd import _lib
from plato_amd import elastic as el
from plato_amd import submodel as sm
from tests import elastic_cases as ec
from tests import elastic_oracle as eo

CASES = ec.load_cases()
NAMES = [c["recipe"]["name"] for c in CASES]


def case_of(name):
    return next(c for c in CASES if c["recipe"]["name"] == name)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(global model, clients) of a fixture case; computed once, shared, never modified."""
    g, clients = ec.build(case_of(name)["recipe"])
    for model in (g, *clients):
        for a in model.values():
            a.setflags(write=False)
    return g, clients


@functools.lru_cache(maxsize=None)
def restated(name):
    g, clients = inputs(name)
    out, counts = eo.aggregate(g, clients, case_of(name)["recipe"]["update_track"])
    for a in out.values():
        a.setflags(write=False)
    return out, counts


@functools.lru_cache(maxsize=None)
def full_arrays(name):
    return ec.load_full(name)


def same_bits(a, b):
    a, b = ec.canon(np.asarray(a)), ec.canon(np.asarray(b))
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_against_fixture(name, result):
    """``result`` (name -> ndarray) is the reference's output of case ``name``: keys, float32 everywhere,
    shapes, hash and samples, and every element where the fixture stores the case in full."""
    case, g = case_of(name), inputs(name)[0]
    exp = case["expected"]
    assert list(result) == list(g)
    assert {k: str(np.asarray(v).dtype) for k, v in result.items()} == exp["dtypes"]
    assert set(exp["dtypes"].values()) == {"float32"}
    for k, v in result.items():
        assert np.asarray(v).shape == g[k].shape, k
    flat = ec.all_flat(result)
    assert flat.size == exp["n_elements"]
    for j, bits in exp["samples"]:
        assert "%08x" % int(flat.view(np.uint32)[j]) == bits, (name, j)
    assert ec.digest(result) == exp["sha"], name
    if case["recipe"]["full"]:
        stored = full_arrays(name)
        assert list(stored) == list(result)
        for k, v in result.items():
            assert same_bits(v, stored[k].reshape(np.asarray(v).shape)), (name, k)


# ------------------------------------------------------------------ the restatement against the reference
@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_reference_bit_for_bit(name):
    out, _ = restated(name)
    check_against_fixture(name, out)
    g = inputs(name)[0]
    counters = [k for k, v in g.items() if v.dtype == np.int64]
    assert counters and all(out[k].dtype == np.float32 and not out[k].any() for k in counters)


def test_the_small_model_is_the_one_the_contract_was_checked_on():
    g, clients = inputs("resnet_small")
    dims = [v.ndim for v in g.values()]
    assert len(g) == 131 and sum(v.size for v in g.values()) == 60439
    assert [dims.count(d) for d in (4, 2, 1, 0)] == [24, 1, 85, 21]
    assert len(clients) == 5 and list(clients[ec.FULL_CLIENT]) == list(g)
    assert len(g) - len(clients[0]) == 24  # depths [2, 2, 2, 2] lack two blocks


def test_fixtures_cover_all_some_and_none_and_an_entry_nobody_holds():
    for case in CASES:
        cov = case["expected"]["coverage"]
        assert cov["all"] > 0 and cov["some"] > 0 and cov["none"] > 0
    unheld = case_of("resnet_small_partial")["expected"]["unheld"]
    assert len(unheld) == 20 and all(k.startswith(("model.layer1.2.", "model.layer3.2.")) for k in unheld)
    assert set(ec.UNHELD) <= set(unheld)
    out, counts = restated("resnet_small_partial")
    g = inputs("resnet_small_partial")[0]
    for k in unheld:  # (g - g) / 1 all over
        with np.errstate(invalid="ignore"):
            assert not counts[k].any() and same_bits(out[k], g[k] - g[k])
    # without update_track the 1-D running statistics are left alone: 2 * (sum of the widths) more elements
    track, no_track = (case_of(n)["expected"]["coverage"]["none"] for n in ("resnet_small", "resnet_small_no_track"))
    g = inputs("resnet_small")[0]
    assert no_track - track == sum(v.size for k, v in g.items() if "running" in k) == 688


def test_special_values_at_covered_uncovered_and_unheld_positions():
    name = "resnet_small_partial"
    out, counts = restated(name)
    g = inputs(name)[0]
    n, k = len(ec.SPECIAL_BITS), len(case_of(name)["recipe"]["clients"])
    pos = ec.special_positions(g)
    got = [out[e].reshape(-1)[at] for e, at, _ in pos]
    cnt = [counts[e].reshape(-1)[at] for e, at, _ in pos]
    big, negz, inf, nan, ninf = got[:n]  # covered by every client
    assert cnt[:n] == [k] * n
    assert big == 0.0  # the clients' values are lost against 1e8
    assert np.isfinite(negz) and negz != 0.0  # -0.0 + x is x
    assert np.isnan(inf) and np.isnan(nan) and np.isnan(ninf)  # inf - inf
    for lo in (n, 2 * n, 3 * n):  # covered by none; held by nobody (twice): (g - g) / 1
        big, negz, inf, nan, ninf = got[lo:lo + n]
        assert not any(cnt[lo:lo + n])
        assert big.tobytes() == negz.tobytes() == np.float32(0.0).tobytes()  # +0, also for g = -0.0
        assert np.isnan(inf) and np.isnan(nan) and np.isnan(ninf)


def test_restatement_keeps_the_order_of_the_clients_and_skips_missing_keys():
    g = OrderedDict(w=np.full(2, 1e8, dtype=np.float32))
    a, b = OrderedDict(w=np.float32([6.0, 6.0])), OrderedDict(w=np.float32([-4.0, 1.0]))
    fwd = eo.aggregate(g, [a, OrderedDict(), b])[0]["w"]
    rev = eo.aggregate(g, [b, a, OrderedDict(other=np.zeros(3, dtype=np.float32))])[0]["w"]
    # against 1e8 (spacing 8): 6 rounds up to 8 and then -4 ties back down to even; -4 first ties to 1e8, then 6 adds 8
    assert fwd[0] == 0.0 and rev[0] == 8.0 / 2.0 and fwd[1] == rev[1] == 8.0 / 2.0


# ------------------------------------------------------------------ ranks and tables
def test_rank_of():
    assert el.rank_of("conv.weight", 4) == 4 and el.rank_of("linear.weight", 2) == 2 and el.rank_of("bn.bias", 1) == 1
    for dim in (0, 3, 5):
        assert el.rank_of("x.weight", dim) == 0 and el.rank_of("x.weight", dim, False) == 0
    for name in ("bn.running_mean", "bn.running_var", "bn.num_batches_tracked"):
        assert el.rank_of(name, 1) == 1 and el.rank_of(name, 1, True) == 1
        assert el.rank_of(name, 1, False) == 0
        assert el.rank_of(name, 2, False) == 2 and el.rank_of(name, 4, False) == 4  # the flag is for 1-D keys
    assert el.rank_of("bn.weight", 1, False) == 1 and el.rank_of("scale", 1, False) == 1
    for name, dim, track in (("a.running_mean", 1, False), ("a.weight", 4, True), ("pos", 3, True), ("s", 0, False)):
        assert el.rank_of(name, dim, track) == eo.rank_of(name, dim, track)


def _toy(update_track=True):
    g, clients = inputs("toy")
    gt, payloads = ec.as_torch(g), [ec.as_torch(c) for c in clients]
    glayout, zeros = el.global_layout(gt)
    sigs = [el.client_signature(glayout, p, update_track, f"p{i}") for i, p in enumerate(payloads)]
    return gt, glayout, zeros, payloads, sigs


def test_tables_of_the_toy_layout():
    gt, glayout, zeros, payloads, sigs = _toy()
    assert zeros == ["norm.num_batches_tracked"]
    assert glayout.keys() == ["pos", "scale", "conv.weight", "conv.bias", "norm.weight", "norm.bias", "norm.running_mean",
                              "norm.running_var", "mix.weight", "extra.weight", "extra.bias", "head.weight", "head.bias"]
    tab = el.build_tables(glayout, sigs)
    assert tab.k == 3 and tab.n_out == glayout.n_f32 == 240 + 1 + 525 + 7 * 5 + 315 + 30 + 6 + 50 + 10
    assert tab.entries.shape == (13, 8) and tab.boxes.shape == (29, 6)
    views = {e.name: tuple(int(v) for v in tab.entries[i, 1:5]) for i, e in enumerate(glayout.entries)}
    assert views == {"pos": (1, 1, 1, 240), "scale": (1, 1, 1, 1),
                     "conv.weight": (7, 3, 5, 5),   # a client is shorter in the kernel dims: the extents stay
                     "conv.bias": (1, 1, 1, 7), "norm.weight": (1, 1, 1, 7), "norm.bias": (1, 1, 1, 7),
                     "norm.running_mean": (1, 1, 1, 7), "norm.running_var": (1, 1, 1, 7),
                     "mix.weight": (1, 1, 5, 63),   # every holder has the 3x3 kernel: one division per element
                     "extra.weight": (1, 1, 6, 5), "extra.bias": (1, 1, 1, 6), "head.weight": (1, 1, 10, 5),
                     "head.bias": (1, 1, 1, 10)}
    assert [int(v) for v in tab.entries[:, 0]] == [e.offset for e in glayout.entries]
    assert [int(v) for v in tab.entries[:, 5]] == list(range(13))  # one tile each
    box = {}
    for i, e in enumerate(glayout.entries):
        first, n = int(tab.entries[i, 6]), int(tab.entries[i, 7])
        box[e.name] = [tuple(int(v) for v in row) for row in tab.boxes[first:first + n]]
    assert [int(v) for v in tab.entries[:, 6]] == list(np.cumsum([0] + [len(b) for b in box.values()])[:-1])
    assert box["pos"] == [] and box["scale"] == []  # rank 0: nobody takes part, no row at all
    assert box["conv.weight"] == [(4, 3, 3, 3, 0, 0), (7, 2, 1, 5, 0, 1), (2, 3, 5, 5, 0, 2)]
    assert box["conv.bias"] == [(1, 1, 1, 4, 108, 0), (1, 1, 1, 7, 70, 1), (1, 1, 1, 2, 150, 2)]
    assert box["norm.running_var"] == [(1, 1, 1, 4, 124, 0), (1, 1, 1, 7, 98, 1), (1, 1, 1, 2, 158, 2)]
    assert box["mix.weight"] == [(1, 1, 3, 36, 128, 0), (1, 1, 5, 63, 105, 1), (1, 1, 2, 18, 160, 2)]
    assert box["extra.weight"] == [(1, 1, 3, 2, 196, 2)] and box["extra.bias"] == [(1, 1, 1, 3, 202, 2)]  # one holder
    assert box["head.weight"] == [(1, 1, 10, 3, 236, 0), (1, 1, 10, 5, 420, 1), (1, 1, 10, 2, 205, 2)]
    assert box["head.bias"] == [(1, 1, 1, 10, 266, 0), (1, 1, 1, 10, 470, 1), (1, 1, 1, 10, 225, 2)]
    assert [int(v) for v in tab.row_len] == [276, 480, 235]
    for i in range(13):  # every box inside its entry's view and its client's row, clients strictly ascending
        rows = tab.boxes[int(tab.entries[i, 6]):int(tab.entries[i, 6] + tab.entries[i, 7])]
        assert (rows[:, :4] <= tab.entries[i, 1:5]).all() and (np.diff(rows[:, 5]) > 0).all()
        for a, b, c, d, src, client in rows:
            assert 0 <= src and src + a * b * c * d <= tab.row_len[client]
    assert tab.covered() == 276 + 480 + 235
    assert tab.algorithmic_bytes() == 4 * (2 * tab.n_out + 276 + 480 + 235)
    assert tab.absent_share() == 1 - 29 / 39
    # without update_track the running statistics have no box and leave the clients' rows
    tab = el.build_tables(glayout, _toy(False)[4], False)
    assert [int(v) for v in tab.row_len] == [276 - 8, 480 - 14, 235 - 4] and len(tab.boxes) == 23
    assert [int(v) for v in tab.entries[6:8, 7]] == [0, 0]


def test_merging_stops_at_the_first_dim_some_holder_cuts():
    g = (6, 4, 5, 5)
    assert el.canonical_view(g, 4, [(6, 4, 5, 5), (2, 4, 5, 5)]) == ((1, 1, 1, 600), [[0, 1, 2, 3]])
    assert el.canonical_view(g, 4, [(6, 4, 5, 5), (2, 3, 5, 5)]) == ((1, 1, 6, 100), [[0], [1, 2, 3]])
    assert el.canonical_view(g, 4, [(6, 4, 3, 5)]) == ((1, 6, 4, 25), [[0], [1], [2, 3]])
    assert el.canonical_view(g, 4, [(6, 4, 5, 3), (6, 4, 5, 5)]) == ((6, 4, 5, 5), [[0], [1], [2], [3]])
    assert el.canonical_view(g, 4, [(6, 4, 5, 5), (6, 2, 3, 5)])[0] == (1, 6, 4, 25)
    assert el.canonical_view(g, 4, []) == ((1, 1, 1, 600), [[0, 1, 2, 3]])  # nobody holds it
    assert el.canonical_view(g, 0, [(6, 4, 5, 5)])[0] == (1, 1, 1, 600)
    assert el.canonical_view((10, 8), 2, [(10, 8), (4, 8)])[0] == (1, 1, 1, 80)
    assert el.canonical_view((10, 8), 2, [(10, 8), (10, 3)])[0] == (1, 1, 10, 8)
    _, groups = el.canonical_view(g, 4, [(2, 3, 5, 5)])
    assert el.client_box(g, groups, (2, 3, 5, 5), "x") == (1, 1, 2, 75)
    assert el.client_box(g, groups, (0, 3, 5, 5), "x") == (1, 1, 0, 75)
    _, groups = el.canonical_view(g, 4, [(2, 3, 1, 5)])
    assert el.client_box(g, groups, (2, 3, 1, 5), "x") == (1, 2, 3, 5)


def test_compact_box_lists_and_tiles():
    g = OrderedDict([("a.weight", torch.zeros(3, 5000)), ("b.bias", torch.zeros(0)), ("c.weight", torch.zeros(4099, 1, 1, 1)),
                     ("d.weight", torch.zeros(4, 4))])
    glayout, zeros = el.global_layout(g)
    p0 = OrderedDict([("a.weight", torch.zeros(3, 0)), ("c.weight", torch.zeros(0, 1, 1, 1)), ("stray", torch.zeros(9))])
    p1 = OrderedDict()  # holds nothing: a row of length 0
    p2 = OrderedDict([("a.weight", torch.zeros(3, 5000)), ("b.bias", torch.zeros(0)), ("c.weight", torch.zeros(4099, 1, 1, 1))])
    tab = el.build_tables(glayout, [el.client_signature(glayout, p, True, "p") for p in (p0, p1, p2)])
    assert not zeros and [int(v) for v in tab.entries[:, 5]] == [0, 15, 15, 20]  # 15 tiles, none, 5, 1
    assert [tuple(int(v) for v in e[1:5]) for e in tab.entries] == [(1, 1, 3, 5000), (1, 1, 1, 0), (1, 1, 1, 4099), (1, 1, 1, 16)]
    assert [(int(e[6]), int(e[7])) for e in tab.entries] == [(0, 2), (2, 1), (3, 2), (5, 0)]  # d.weight: held by nobody
    assert [tuple(int(v) for v in b) for b in tab.boxes] == [
        (1, 1, 3, 0, 0, 0), (1, 1, 3, 5000, 0, 2), (1, 1, 1, 0, 15000, 2), (1, 1, 1, 0, 0, 0), (1, 1, 1, 4099, 15000, 2)]
    assert [int(v) for v in tab.row_len] == [0, 0, 19099] and tab.absent_share() == 1 - 5 / 12


# ------------------------------------------------------------------ the Python refusals
def _round(g, payloads, update_track=True, engine=None):
    return el.ElasticRound(engine or object(), g, payloads, update_track)  # the constructor touches no GPU


def test_python_refusals_come_before_any_staging():
    g, _, _, payloads, _ = _toy()
    assert len(_round(g, payloads).tables.boxes) == 29
    with pytest.raises(ValueError, match="no client payloads"):
        _round(g, [])
    with pytest.raises(ValueError, match="at most 4096 clients"):
        _round(g, [payloads[0]] * 4097)
    assert el.MAX_K == 4096 == _lib.PLATO_AGG_ELASTIC_MAX_K
    coded = OrderedDict((k, v.to(torch.bfloat16)) for k, v in payloads[0].items())
    with pytest.raises(ValueError, match="native payloads"):
        _round(g, [payloads[0], coded])
    qsgd = OrderedDict(payloads[0])
    qsgd.plato_codec = "qsgd"
    with pytest.raises(ValueError, match="native payloads"):
        _round(g, [qsgd])
    with pytest.raises(NotImplementedError, match="one GPU"):
        _round(g, payloads, engine=types.SimpleNamespace(primary=object()))
    dims = OrderedDict(payloads[0], **{"norm.bias": torch.zeros(4, 1)})
    with pytest.raises(ValueError, match=r"weights_received\[1\]\['norm.bias'\] has 2 dims"):
        _round(g, [payloads[0], dims])
    for key, shape in (("conv.weight", (8, 3, 3, 3)), ("conv.weight", (4, 3, 6, 3)), ("conv.weight", (4, 3, 3, 6)),
                       ("head.weight", (10, 6)), ("norm.running_mean", (8,))):
        with pytest.raises(ValueError, match="an extent above the global's"):
            _round(g, [OrderedDict(payloads[0], **{key: torch.zeros(shape)})])
    for dtype in (torch.float64, torch.int64, torch.float16):
        half = OrderedDict(payloads[0], **{"norm.running_var": torch.zeros(4, dtype=dtype)})
        with pytest.raises(ValueError, match="expected torch.float32"):
            _round(g, [half])
        _round(g, [half], update_track=False)  # rank 0 now: never read
        with pytest.raises(ValueError, match="elastic aggregation takes torch.float32 entries"):
            _round(OrderedDict(g, **{"norm.weight": torch.zeros(7, dtype=dtype)}), payloads)
    for shape in ((3,), (3, 3), (1, 1, 1, 1)):  # an integer entry that clients could cover is not built
        with pytest.raises(ValueError, match="integer entries whose dim is not 1, 2 or 4"):
            _round(OrderedDict(g, **{"norm.num_batches_tracked": torch.zeros(shape, dtype=torch.int64)}), payloads)
    with pytest.raises(ValueError, match="elastic aggregation takes torch.float32 entries"):
        _round(OrderedDict(g, flag=torch.zeros((), dtype=torch.bool)), payloads)
    # legal: keys of rank 0 are never read, whatever they hold; keys that the global model lacks are ignored; a
    # client may hold nothing; an extent of 0 covers nothing; an int32 counter of 3 dims is zeros like a 0-D one
    odd = OrderedDict(payloads[0], pos=torch.zeros(9, 9, dtype=torch.int64), scale="nothing", stray=torch.zeros(2, 2))
    assert _round(g, [odd]).signatures == _round(g, [payloads[0]]).signatures
    rnd = _round(g, [payloads[0], OrderedDict(), payloads[2]])
    assert [int(v) for v in rnd.tables.row_len] == [276, 0, 235] and len(rnd.tables.boxes) == 9 + 11
    zero = OrderedDict(payloads[0], **{"conv.weight": torch.zeros(4, 0, 3, 3)})
    assert tuple(int(v) for v in _round(g, [zero]).tables.boxes[0]) == (4, 0, 3, 3, 0, 0)
    assert _round(OrderedDict(g, steps=torch.zeros(2, 1, 2, dtype=torch.int32)), payloads).zeros == [
        "norm.num_batches_tracked", "steps"]


def test_multi_device_engine_refuses_elastic_rounds():
    from plato_amd.multi import MultiDeviceEngine

    with pytest.raises(NotImplementedError, match="one GPU"):
        MultiDeviceEngine.aggregate_elastic(object(), {}, [])
    with pytest.raises(NotImplementedError, match="one GPU"):
        MultiDeviceEngine.begin_elastic(object(), {}, [])


def test_the_width_only_module_still_refuses_this_rule():
    assert "sysheterofl" not in sm.RULES and sorted(sm.RULES) == ["fedrolex", "heterofl"]
    with pytest.raises(ValueError, match="unknown sub-model rule"):
        sm.prefix_rank("sysheterofl", "conv.weight", 4)
    with pytest.raises(ValueError, match="unknown sub-model rule"):
        sm.SubmodelRound(object(), {}, [{}], "sysheterofl")


# ------------------------------------------------------------------ hook (stub engine)
class _Round:
    def __init__(self, log):
        self.log, self.timings = log, {}

    def stage(self):
        self.log.append("stage")

    def launch(self):
        self.log.append("launch")

    def wait(self):
        pass

    def result(self):
        return {"w": 1}

    def algorithmic_bytes(self):
        return 0


class _Engine:
    def __init__(self):
        self.log, self.released = [], 0

    def begin_elastic(self, global_model, payloads, update_track=True):
        self.log.append(("begin", global_model, list(payloads), update_track))
        return _Round(self.log)

    def release_arrivals(self):
        self.released += 1


def _server():
    from plato_amd.servers import ElasticAggregationMixin

    s = type("Server", (ElasticAggregationMixin,), {})()
    s._plato_amd_engine = _Engine()
    s.algorithm = types.SimpleNamespace(model=types.SimpleNamespace(state_dict=lambda: {"the": "model"}))
    return s


def test_hook_reads_the_algorithms_model():
    payloads = [{"w": torch.zeros(2)}]
    s = _server()
    got = asyncio.run(s.aggregate_weights([], {"not": "read"}, payloads))
    assert got == {"w": 1}
    assert s._plato_amd_engine.log == [("begin", {"the": "model"}, payloads, True), "stage", "launch"]
    assert s._plato_amd_engine.released == 1


def test_hook_refuses_several_devices_before_any_engine_call():
    s = _server()
    s._plato_amd_engine.primary = object()  # what a multi-GPU engine carries
    with pytest.raises(NotImplementedError, match="one GPU"):
        asyncio.run(s.aggregate_weights([], {}, [{"w": torch.zeros(2)}]))
    assert s._plato_amd_engine.log == [] and s._plato_amd_engine.released == 0


def test_hook_releases_arrivals_when_a_refusal_is_raised():
    s = _server()
    s._plato_amd_engine.begin_elastic = lambda *a: (_ for _ in ()).throw(ValueError("no client payloads"))
    with pytest.raises(ValueError, match="no client payloads"):
        asyncio.run(s.aggregate_weights([], {}, []))
    assert s._plato_amd_engine.released == 1


# ------------------------------------------------------------------ ABI
def _tables(entries, boxes, row_len):
    e = np.ascontiguousarray(entries, dtype=np.int64).reshape(-1, 8)
    b = np.ascontiguousarray(boxes, dtype=np.int64).reshape(-1, 6)
    r = np.ascontiguousarray(row_len, dtype=np.int64)
    return e, b, r


def test_elastic_argument_errors_are_raised_without_gpu_work():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = _lib.lib()
    a = 1 << 12  # an aligned non-null address: nothing on the device is dereferenced on these paths
    size = lib.plato_agg_elastic_tables_bytes
    assert size((1 << 20) + 1, 4) == 0 and size(1, (1 << 32) + 1) == 0
    assert size(0, 0) == 256 and size(1, 0) == 256 and size(1, 1) == 512 and size(4, 0) == 256 and size(5, 0) == 512
    assert size(6, 18) == 512 + 1024  # 6 * 64 bytes of entries rounded up to 256, then 18 boxes of 48

    # two entries, [1, 2, 1, 3] at offset 0 and [1, 1, 1, 4] at 6; three clients with rows of 6, 4 and 5 elements;
    # the first entry is held by clients 0 and 2, the second by client 1
    e, b, r = _tables([[0, 1, 2, 1, 3, 0, 0, 2], [6, 1, 1, 1, 4, 1, 2, 1]],
                      [[1, 2, 1, 3, 0, 0], [1, 2, 1, 2, 1, 2], [1, 1, 1, 4, 0, 1]], [6, 4, 5])

    def call(d_global=a, d_rows=a, k=3, row_len=r, entries=e, n_entries=None, boxes=b, n_boxes=None, d_tables=a,
             d_out=a, n_out=10):
        ptr = lambda x: x if x is None or isinstance(x, int) else x.ctypes.data  # noqa: E731
        n_entries = n_entries if n_entries is not None else (0 if entries is None or isinstance(entries, int) else len(entries))
        n_boxes = n_boxes if n_boxes is not None else (0 if boxes is None or isinstance(boxes, int) else len(boxes))
        _lib.call("plato_agg_elastic_mean", d_global, d_rows, k, ptr(row_len), ptr(entries), n_entries, ptr(boxes),
                  n_boxes, d_tables, d_out, n_out, None)

    for k in (0, 4097, -3):
        with pytest.raises(ValueError, match=r"K must be in 1\.\.4096"):
            call(k=k)
    with pytest.raises(ValueError, match="2\\^20 entries"):
        call(n_entries=(1 << 20) + 1)
    with pytest.raises(ValueError, match="2\\^32 boxes"):
        call(n_boxes=(1 << 32) + 1)
    for kw in ({"d_global": None}, {"d_out": None}):
        with pytest.raises(ValueError, match="null fp32 arena pointer"):
            call(**kw)
    for kw in ({"d_rows": None}, {"row_len": None}):
        with pytest.raises(ValueError, match="null client row table"):
            call(**kw)
    for kw in ({"entries": None, "n_entries": 2}, {"boxes": None, "n_boxes": 3}, {"d_tables": None}):
        with pytest.raises(ValueError, match="null entry or box table"):
            call(**kw)
    for kw in ({"d_rows": a + 4}, {"row_len": r.ctypes.data + 4}, {"entries": e.ctypes.data + 4, "n_entries": 2},
               {"boxes": b.ctypes.data + 4, "n_boxes": 3}):
        with pytest.raises(ValueError, match="8-byte aligned"):
            call(**kw)
    with pytest.raises(ValueError, match="256-byte aligned"):
        call(d_tables=a + 128)
    with pytest.raises(ValueError, match="4-byte aligned"):
        call(d_global=a + 2)
    with pytest.raises(ValueError, match="16-byte aligned"):
        call(d_out=a + 4)
    with pytest.raises(ValueError, match="2\\^38"):
        call(n_out=1 << 38)
    call(entries=None, boxes=None)  # nothing to do: no launch, no error
    call(n_out=0, d_global=None, d_out=None)

    def bad(match, entries=e, boxes=b, row_len=r, k=3, n_out=10):
        with pytest.raises(ValueError, match=match):
            call(entries=_tables(entries, b, r)[0], boxes=_tables(e, boxes, r)[1], row_len=_tables(e, b, row_len)[2],
                 k=k, n_out=n_out)

    def entry(i, **words):  # the entry table with words of row i replaced
        rows, col = e.copy(), dict(out=0, A=1, B=2, C=3, D=4, tile0=5, box0=6, n_boxes=7)
        for name, v in words.items():
            rows[i, col[name]] = v
        return rows

    def box(i, **words):
        rows, col = b.copy(), dict(a=0, b=1, c=2, d=3, src=4, client=5)
        for name, v in words.items():
            rows[i, col[name]] = v
        return rows

    bad("row length outside", row_len=[6, -1, 5])
    bad("row length outside", row_len=[1 << 38, 4, 5])
    bad("entry 0: bad view extents", entries=entry(0, B=-2))
    bad("entry 0: bad view extents", entries=entry(0, A=1 << 20, B=1 << 20))
    bad("entry 0: output range", entries=entry(0, out=-1))
    bad("entry 1: output range", n_out=9)
    bad("entry 1: output range", entries=entry(1, out=5))          # starts inside the first entry
    bad("entry 0: first tile", entries=entry(0, tile0=1))
    bad("entry 1: first tile", entries=entry(1, tile0=0))          # claims the first entry's tile
    bad("entry 1: first tile", entries=entry(1, tile0=2))
    bad("entry 1: box range", entries=entry(1, box0=3, n_boxes=0))  # a gap: box 2 belongs to nobody
    bad("entry 1: box range", entries=entry(1, box0=1))            # shares a box with the first entry
    bad("entry 0: box range", entries=entry(0, n_boxes=4))         # runs past the table
    bad("entry 0: box range", entries=entry(0, n_boxes=-1))
    bad("box ranges end before the box table", entries=entry(1, n_boxes=0))
    bad("entry 0, box 1: clients are not strictly ascending", boxes=box(0, client=2, d=2))
    bad("entry 0, box 1: clients are not strictly ascending", boxes=box(1, client=0, src=0))
    for client in (3, -1):
        bad("entry 1, box 0: client outside", boxes=box(2, client=client))
    bad("entry 0, box 1: client outside", boxes=box(1, client=2), k=2)
    for words in (dict(a=2), dict(b=3), dict(c=2), dict(d=4), dict(d=-1)):
        bad("entry 0, box 0: box extent above the entry's extent", boxes=box(0, **words))
    bad("entry 0, box 1: box runs past the client's row length", boxes=box(1, src=2))
    bad("entry 0, box 1: box runs past the client's row length", boxes=box(1, d=3))
    bad("entry 0, box 0: box runs past the client's row length", boxes=box(0, src=7))
    bad("entry 1, box 0: box runs past the client's row length", boxes=box(2, d=0, src=5))
    bad("entry 0, box 1: box runs past the client's row length", boxes=box(1, src=-2))
    # entries without elements, a box that covers nothing and a client with an empty row: accepted, nothing to launch
    call(entries=_tables([[0, 1, 0, 1, 3, 0, 0, 2], [6, 1, 1, 1, 0, 0, 2, 1]], b, r)[0],
         boxes=_tables(e, [[1, 0, 1, 3, 6, 0], [0, 0, 0, 0, 0, 1], [1, 1, 1, 0, 5, 2]], r)[1],
         row_len=_tables(e, b, [6, 0, 5])[2])


def test_constants_match_the_header():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "plato_agg.h")).read()
    for name in ("MAX_K", "TILE", "ENTRY_WORDS", "BOX_WORDS"):
        value = getattr(_lib, "PLATO_AGG_ELASTIC_" + name)
        assert f"#define PLATO_AGG_ELASTIC_{name} {value}\n" in text
    assert (el.ENTRY_WORDS, el.BOX_WORDS, el.TILE) == (8, 6, 1024)
    assert "#define PLATO_AGG_ELASTIC_MAX_ENTRIES 1048576\n" in text
