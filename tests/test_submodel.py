"""Sub-model aggregation without a GPU: the numpy restatement (tests/submodel_oracle.py) against the
reference fixtures (tests/golden/submodel_*) bit for bit, prefix ranks and the table builder
(plato_amd.submodel), every refusal of plato_agg_submodel_mean and of the Python layer, and the hook on a
stub engine."""

import asyncio
import functools
import os
import types
from collections import OrderedDict

import numpy as np
import pytest
import torch

from plato_amd import _lib
from plato_amd import submodel as sm
from plato_amd.arena import ArenaLayout
from tests import submodel_cases as sc
from tests import submodel_oracle as so

CASES = sc.load_cases()
NAMES = [c["recipe"]["name"] for c in CASES]


def case_of(name):
    return next(c for c in CASES if c["recipe"]["name"] == name)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(global model, clients) of a fixture case; computed once, shared, never modified."""
    g, clients = sc.build(case_of(name)["recipe"])
    for model in (g, *clients):
        for a in model.values():
            a.setflags(write=False)
    return g, clients


@functools.lru_cache(maxsize=None)
def restated(name):
    g, clients = inputs(name)
    out, counts = so.aggregate(g, clients, case_of(name)["recipe"]["rule"])
    for a in out.values():
        a.setflags(write=False)
    return out, counts


@functools.lru_cache(maxsize=None)
def full_arrays():
    return sc.load_full()


def same_bits(a, b):
    a, b = sc.canon(np.asarray(a)), sc.canon(np.asarray(b))
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_against_fixture(name, result):
    """``result`` (name -> ndarray) is the reference's output of case ``name``: dtypes, hash and samples,
    and every element where the fixture stores the case in full."""
    case, g = case_of(name), inputs(name)[0]
    exp = case["expected"]
    assert list(result) == list(g)
    assert {k: str(np.asarray(v).dtype) for k, v in result.items()} == exp["dtypes"]
    for k, v in result.items():
        assert np.asarray(v).shape == g[k].shape, k
    flat = sc.participating_flat(result)
    assert flat.size == exp["n_participating"]
    for j, bits in exp["samples"]:
        assert "%08x" % int(flat.view(np.uint32)[j]) == bits, (name, j)
    assert sc.digest(result) == exp["sha"], name
    if case["recipe"]["full"]:
        stored = full_arrays()
        for k, v in result.items():
            assert same_bits(v, stored[name + "|" + k].reshape(np.asarray(v).shape)), (name, k)


# ------------------------------------------------------------------ the restatement against the reference
@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_reference_bit_for_bit(name):
    out, _ = restated(name)
    check_against_fixture(name, out)
    g = inputs(name)[0]
    for k, v in out.items():  # entries that pass through keep the global model's dtype and bits
        if not so.participates(k):
            assert v.dtype == g[k].dtype and v.tobytes() == g[k].tobytes(), k
    assert any(v.dtype == np.int64 for v in out.values())


def test_fixtures_cover_all_some_and_none():
    for case in CASES:
        cov, rec = case["expected"]["coverage"], case["recipe"]
        assert cov["all"] > 0 and cov["some"] > 0
        if rec["name"] != "resnet18_small":  # its full-width client covers every element
            assert cov["none"] > 0
    toy = {c["recipe"]["algo"]: c["expected"]["coverage"]["none"] for c in CASES if c["recipe"]["model"] == "toy"}
    # the two rules differ on the 3-D entry: 5 * 6 * 8 uncovered elements under "heterofl", the 0-D one under both
    assert toy["heterofl"] == toy["fjord"] == 241 and toy["fedrolex"] == toy["anycostfl"] == 1


def test_special_values_at_covered_and_uncovered_positions():
    name = "resnet18_small_special"
    out, counts = restated(name)
    flat = out[sc.SPECIAL_ENTRY].reshape(-1)
    cnt = counts[sc.SPECIAL_ENTRY].reshape(-1)
    n, k = len(sc.SPECIAL_BITS), len(case_of(name)["recipe"]["client_rates"])
    pos = sc.special_positions(flat.size)
    big, negz, inf, nan, ninf = (flat[at] for at, _ in pos[:n])  # covered by every client
    assert all(cnt[at] == k for at, _ in pos[:n])
    assert big == 0.0  # the clients' values are lost against 1e8: (1e8 + x... - 1e8) / K
    assert np.isfinite(negz) and negz != 0.0  # -0.0 + x is x
    assert np.isnan(inf) and np.isnan(nan) and np.isnan(ninf)  # inf - inf
    big, negz, inf, nan, ninf = (flat[at] for at, _ in pos[n:])  # covered by none: (g - g) / 1
    assert all(cnt[at] == 0 for at, _ in pos[n:])
    assert big.tobytes() == negz.tobytes() == np.float32(0.0).tobytes()  # +0, also for g = -0.0
    assert np.isnan(inf) and np.isnan(nan) and np.isnan(ninf)


def test_restatement_keeps_the_order_of_the_clients():
    g = OrderedDict(weight=np.zeros(2, dtype=np.float32))
    xs = [OrderedDict(weight=np.float32([v, v])) for v in (1e8, 1.0, -1e8)]
    fwd = so.aggregate(g, xs, "heterofl")[0]["weight"]
    rev = so.aggregate(g, [xs[1], xs[0], xs[2]], "heterofl")[0]["weight"]
    assert fwd[0] == 0.0 and rev[0] == 0.0  # 1 is lost either way here ...
    xs = [OrderedDict(weight=np.float32([v, v])) for v in (1e8, -1e8, 1.0)]
    assert so.aggregate(g, xs, "heterofl")[0]["weight"][0] == np.float32(1.0) / np.float32(3.0)  # ... not here


# ------------------------------------------------------------------ prefix ranks and tables
def test_prefix_rank():
    for rule in ("heterofl", "fedrolex"):
        assert sm.prefix_rank(rule, "conv.weight", 4) == 2
        assert sm.prefix_rank(rule, "linear.weight", 2) == 2
        assert sm.prefix_rank(rule, "bn.bias", 1) == 1
        assert sm.prefix_rank(rule, "s_bias", 0) == 0
        assert sm.prefix_rank(rule, "x.weight", 5) == 0
        for name in ("bn.running_mean", "bn.running_var", "bn.num_batches_tracked", "scale"):
            assert sm.prefix_rank(rule, name, 1) is None
    assert sm.prefix_rank("heterofl", "pos_weight", 3) == 0
    assert sm.prefix_rank("fedrolex", "pos_weight", 3) == 3
    with pytest.raises(ValueError, match="unknown sub-model rule"):
        sm.prefix_rank("sysheterofl", "conv.weight", 4)


def _toy(rate, rule, extra_rates=()):
    g = sc.as_torch(sc.fill(sc.toy_spec(1.0), 5, 0))
    glayout = sm.global_layout(g)
    payloads = [sc.as_torch(sc.fill(sc.toy_spec(r), 5, 1 + i)) for i, r in enumerate((rate, *extra_rates))]
    sigs = [sm.client_signature(glayout, rule, p, f"p{i}") for i, p in enumerate(payloads)]
    return g, glayout, payloads, sigs


def test_tables_of_the_toy_layout():
    g, glayout, payloads, sigs = _toy(0.5, "fedrolex", (1.0, 0.125))
    assert glayout.keys() == ["pos_weight", "s_bias", "stem.weight", "norm.weight", "norm.bias", "mix.weight",
                              "mix.bias", "head.weight", "head.bias"]
    tab = sm.build_tables(glayout, sigs, "fedrolex")
    assert tab.k == 3 and tab.n_out == glayout.n_f32 == 240 + 1 + 189 + 7 + 7 + 91 + 13 + 130 + 10
    views = {e.name: tuple(tab.entries[i, 1:4]) for i, e in enumerate(glayout.entries)}
    assert views == {"pos_weight": (5, 6, 8), "s_bias": (1, 1, 1), "stem.weight": (7, 1, 27), "norm.weight": (1, 1, 7),
                     "norm.bias": (1, 1, 7), "mix.weight": (13, 1, 7), "mix.bias": (1, 1, 13),
                     "head.weight": (10, 1, 13), "head.bias": (1, 1, 10)}
    assert [int(v) for v in tab.entries[:, 0]] == [e.offset for e in glayout.entries]
    assert [int(v) for v in tab.entries[:, 4]] == list(range(len(glayout.entries)))  # one tile each
    assert not tab.entries[:, 5].any()
    box = {e.name: [tuple(int(v) for v in tab.boxes[i, c]) for c in range(3)] for i, e in enumerate(glayout.entries)}
    # rate 0.5: widths 4 and 7, pos (3, 3, 4); rate 1: the global's; rate 0.125: 1 and 2, pos (1, 1, 1)
    assert box["pos_weight"] == [(3, 3, 4, 0), (5, 6, 8, 0), (1, 1, 1, 0)]
    assert box["s_bias"] == [(0, 0, 0, sm.ABSENT)] * 3  # rank 0: no client covers it
    assert box["stem.weight"] == [(4, 1, 27, 36), (7, 1, 27, 240), (1, 1, 27, 1)]
    assert box["norm.weight"] == [(1, 1, 4, 144), (1, 1, 7, 429), (1, 1, 1, 28)]
    assert box["mix.weight"] == [(7, 1, 4, 152), (13, 1, 7, 443), (2, 1, 1, 30)]
    assert box["head.weight"] == [(10, 1, 7, 187), (10, 1, 13, 547), (10, 1, 2, 34)]  # dim 0 is full at every rate
    assert box["head.bias"] == [(1, 1, 10, 257), (1, 1, 10, 677), (1, 1, 10, 54)]
    assert [int(v) for v in tab.row_len] == [267, 687, 64]
    for i in range(len(glayout.entries)):  # every box inside its entry's view and its client's row
        for c in range(3):
            p, q, l, src = (int(v) for v in tab.boxes[i, c])
            if src != sm.ABSENT:
                assert p <= tab.entries[i, 1] and q <= tab.entries[i, 2] and l <= tab.entries[i, 3]
                assert 0 <= src and src + p * q * l <= tab.row_len[c]
    assert tab.covered() == 267 + 687 + 64
    assert tab.algorithmic_bytes() == 4 * (2 * tab.n_out + 267 + 687 + 64)
    # under "heterofl" the 3-D entry has rank 0: no box, and the clients' rows do not hold it
    tab = sm.build_tables(glayout, [sm.client_signature(glayout, "heterofl", p, "p") for p in payloads], "heterofl")
    assert [tuple(int(v) for v in tab.boxes[0, c]) for c in range(3)] == [(0, 0, 0, sm.ABSENT)] * 3
    assert tuple(tab.entries[0, 1:4]) == (1, 1, 240)
    assert [int(v) for v in tab.row_len] == [267 - 36, 687 - 240, 64 - 1]


def test_tables_take_zero_and_full_extents_and_count_tiles():
    g = OrderedDict([("a.weight", torch.zeros(3, 5000)), ("b.bias", torch.zeros(0)), ("c.weight", torch.zeros(4099, 1, 1, 1))])
    glayout = sm.global_layout(g)
    p0 = OrderedDict([("a.weight", torch.zeros(3, 0)), ("b.bias", torch.zeros(0)), ("c.weight", torch.zeros(0, 1, 1, 1))])
    p1 = OrderedDict([("a.weight", torch.zeros(3, 5000)), ("b.bias", torch.zeros(0)), ("c.weight", torch.zeros(4099, 1, 1, 1))])
    tab = sm.build_tables(glayout, [sm.client_signature(glayout, "heterofl", p, "p") for p in (p0, p1)], "heterofl")
    assert [int(v) for v in tab.entries[:, 4]] == [0, 15, 15]  # ceil(15000 / 1024) tiles, then an empty entry
    assert [tuple(int(v) for v in tab.boxes[i, 0]) for i in range(3)] == [(3, 1, 0, 0), (1, 1, 0, 0), (0, 1, 1, 0)]
    assert [tuple(int(v) for v in tab.boxes[i, 1]) for i in range(3)] == [(3, 1, 5000, 0), (1, 1, 0, 15000),
                                                                           (4099, 1, 1, 15000)]
    assert [int(v) for v in tab.row_len] == [0, 19099]


# ------------------------------------------------------------------ the Python refusals
def _round(g, payloads, rule="heterofl"):
    return sm.SubmodelRound(object(), g, payloads, rule)  # the constructor touches no engine and no GPU


def test_python_refusals_come_before_any_staging():
    g, _, payloads, _ = _toy(0.5, "fedrolex", (0.25,))
    _round(g, payloads, "fedrolex")
    with pytest.raises(ValueError, match="no client payloads"):
        _round(g, [])
    with pytest.raises(ValueError, match="unknown sub-model rule"):
        _round(g, payloads, "sysheterofl")
    with pytest.raises(ValueError, match="at most 4096 clients"):
        _round(g, [payloads[0]] * 4097)
    missing = OrderedDict((k, v) for k, v in payloads[0].items() if k != "mix.weight")
    with pytest.raises(ValueError, match=r"weights_received\[1\] is missing 'mix.weight'"):
        _round(g, [payloads[0], missing])
    # pass-through keys and rank-0 entries are never read: they may be absent
    bare = OrderedDict((k, v) for k, v in payloads[0].items()
                       if so.participates(k) and k not in ("s_bias", "pos_weight"))
    _round(g, [bare], "heterofl")
    with pytest.raises(ValueError, match="missing 'pos_weight'"):
        _round(g, [bare], "fedrolex")
    wide = OrderedDict(payloads[0], **{"stem.weight": torch.zeros(8, 3, 3, 3)})
    with pytest.raises(ValueError, match="an extent above the global's"):
        _round(g, [wide])
    wide = OrderedDict(payloads[0], **{"head.weight": torch.zeros(10, 14)})
    with pytest.raises(ValueError, match="an extent above the global's"):
        _round(g, [wide])
    trailing = OrderedDict(payloads[0], **{"stem.weight": torch.zeros(4, 3, 3, 2)})
    with pytest.raises(ValueError, match="trailing dims differ"):
        _round(g, [trailing])
    dims = OrderedDict(payloads[0], **{"norm.bias": torch.zeros(4, 1)})
    with pytest.raises(ValueError, match="has 2 dims"):
        _round(g, [dims])
    half = OrderedDict(payloads[0], **{"norm.bias": torch.zeros(4, dtype=torch.float64)})
    with pytest.raises(ValueError, match="expected torch.float32"):
        _round(g, [half])
    with pytest.raises(ValueError, match="participating entries are torch.float32"):
        _round(OrderedDict(g, **{"norm.weight": torch.zeros(7, dtype=torch.float64)}), payloads)
    coded = OrderedDict((k, v.to(torch.bfloat16)) for k, v in payloads[0].items())
    with pytest.raises(ValueError, match="native payloads"):
        _round(g, [payloads[0], coded])
    qsgd = OrderedDict(payloads[0])
    qsgd.plato_codec = "qsgd"
    with pytest.raises(ValueError, match="native payloads"):
        _round(g, [qsgd])
    zero = OrderedDict(payloads[0], **{"stem.weight": torch.zeros(0, 3, 3, 3)})  # legal: covers nothing
    assert tuple(_round(g, [zero]).tables.boxes[2, 0][:3]) == (0, 1, 27)


def test_multi_device_engine_refuses_submodels():
    from plato_amd.multi import MultiDeviceEngine

    with pytest.raises(NotImplementedError, match="one GPU"):
        MultiDeviceEngine.aggregate_submodels(object(), {}, [])
    with pytest.raises(NotImplementedError, match="one GPU"):
        MultiDeviceEngine.begin_submodels(object(), {}, [])


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

    def begin_submodels(self, global_model, payloads, rule="heterofl"):
        self.log.append(("begin", global_model, list(payloads), rule))
        return _Round(self.log)

    def release_arrivals(self):
        self.released += 1


def _server(**attrs):
    from plato_amd.servers import SubmodelAggregationMixin

    s = type("Server", (SubmodelAggregationMixin,), attrs)()
    s._plato_amd_engine = _Engine()
    s.algorithm = types.SimpleNamespace(model=types.SimpleNamespace(state_dict=lambda: {"the": "model"}))
    return s


def test_hook_reads_the_algorithms_model_and_passes_the_rule():
    payloads = [{"w": torch.zeros(2)}]
    for attrs, rule in (({}, "heterofl"), ({"submodel_rule": "fedrolex"}, "fedrolex")):
        s = _server(**attrs)
        got = asyncio.run(s.aggregate_weights([], {"not": "read"}, payloads))
        assert got == {"w": 1}
        assert s._plato_amd_engine.log == [("begin", {"the": "model"}, payloads, rule), "stage", "launch"]
        assert s._plato_amd_engine.released == 1


def test_hook_refuses_several_devices_before_any_engine_call():
    s = _server()
    s._plato_amd_engine.primary = object()  # what a multi-GPU engine carries
    with pytest.raises(NotImplementedError, match="one GPU"):
        asyncio.run(s.aggregate_weights([], {}, [{"w": torch.zeros(2)}]))
    assert s._plato_amd_engine.log == [] and s._plato_amd_engine.released == 0


def test_hook_releases_arrivals_when_a_refusal_is_raised():
    s = _server()
    s._plato_amd_engine.begin_submodels = lambda *a: (_ for _ in ()).throw(ValueError("no client payloads"))
    with pytest.raises(ValueError, match="no client payloads"):
        asyncio.run(s.aggregate_weights([], {}, []))
    assert s._plato_amd_engine.released == 1


# ------------------------------------------------------------------ ABI
def _tables(entries, boxes, row_len):
    e = np.ascontiguousarray(entries, dtype=np.int64)
    b = np.ascontiguousarray(boxes, dtype=np.int64)
    r = np.ascontiguousarray(row_len, dtype=np.int64)
    return e, b, r


def test_submodel_argument_errors_are_raised_without_gpu_work():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = _lib.lib()
    a = 1 << 12  # an aligned non-null address: nothing on the device is dereferenced on these paths
    assert _lib.ABI_VERSION == 5 and lib.plato_agg_abi_version() == 5
    size = lib.plato_agg_submodel_tables_bytes
    assert size(0, 4) == 0 and size(4097, 4) == 0 and size(-1, 4) == 0 and size(2, (1 << 20) + 1) == 0
    assert size(2, 0) == 256 and size(1, 1) == 512 and size(4096, 1) == 256 + 4096 * 32
    assert size(3, 6) == 512 + 768  # 6 * 48 bytes of entries rounded up to 256, then 18 boxes of 32

    # one entry [2, 1, 3] at offset 0, two clients: rows of 6 and 4 elements
    e, b, r = _tables([[0, 2, 1, 3, 0, 0]], [[[2, 1, 3, 0], [2, 1, 2, 0]]], [6, 4])

    def call(d_global=a, d_rows=a, k=2, row_len=r, entries=e, boxes=b, n_entries=1, d_tables=a, d_out=a, n_out=6):
        ptr = lambda x: x if x is None or isinstance(x, int) else x.ctypes.data  # noqa: E731
        _lib.call("plato_agg_submodel_mean", d_global, d_rows, k, ptr(row_len), ptr(entries), ptr(boxes), n_entries,
                  d_tables, d_out, n_out, None)

    for k in (0, 4097, -3):
        with pytest.raises(ValueError, match=r"K must be in 1\.\.4096"):
            call(k=k)
    with pytest.raises(ValueError, match="2\\^20 entries"):
        call(n_entries=(1 << 20) + 1)
    for kw in ({"d_global": None}, {"d_out": None}):
        with pytest.raises(ValueError, match="null fp32 arena pointer"):
            call(**kw)
    for kw in ({"d_rows": None}, {"row_len": None}):
        with pytest.raises(ValueError, match="null client row table"):
            call(**kw)
    for kw in ({"entries": None}, {"boxes": None}, {"d_tables": None}):
        with pytest.raises(ValueError, match="null entry or box table"):
            call(**kw)
    for kw in ({"d_rows": a + 4}, {"row_len": r.ctypes.data + 4}, {"entries": e.ctypes.data + 4},
               {"boxes": b.ctypes.data + 4}):
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
    call(n_entries=0, entries=None, boxes=None)  # nothing to do: no launch, no error
    call(n_out=0, d_global=None, d_out=None)

    def bad(match, entries=e, boxes=b, row_len=r, n_out=6):
        with pytest.raises(ValueError, match=match):
            call(entries=entries, boxes=boxes, row_len=row_len, n_out=n_out, n_entries=len(entries))

    bad("row length outside", row_len=_tables(e, b, [6, -1])[2])
    bad("row length outside", row_len=_tables(e, b, [1 << 38, 4])[2])
    bad("entry 0: bad view extents", entries=_tables([[0, -2, 1, 3, 0, 0]], b, r)[0])
    bad("entry 0: bad view extents", entries=_tables([[0, 1 << 20, 1 << 20, 3, 0, 0]], b, r)[0])
    bad("entry 0: output range", entries=_tables([[-1, 2, 1, 3, 0, 0]], b, r)[0])
    bad("entry 0: output range", n_out=5)
    bad("entry 0: output range", entries=_tables([[1, 2, 1, 3, 0, 0]], b, r)[0])
    bad("entry 0: first tile", entries=_tables([[0, 2, 1, 3, 1, 0]], b, r)[0])
    bad("entry 0: first tile", entries=_tables([[0, 2, 1, 3, 0, 7]], b, r)[0])
    two = [[0, 2, 1, 3, 0, 0], [4, 1, 1, 2, 1, 0]]  # the second entry starts inside the first
    bad("entry 1: output range", entries=_tables(two, b, r)[0], boxes=np.concatenate([b, b]), n_out=8)
    two = [[0, 2, 1, 3, 0, 0], [6, 1, 1, 2, 0, 0]]  # ... or claims the first entry's tile
    bad("entry 1: first tile", entries=_tables(two, b, r)[0], boxes=np.concatenate([b, b]), n_out=8)
    for box in ([3, 1, 3, 0], [2, 2, 3, 0], [2, 1, 4, 0], [-1, 1, 3, 0]):
        bad("entry 0, client 1: box extent above the global's extent", boxes=_tables(e, [[[2, 1, 3, 0], box]], r)[1])
    bad("entry 0, client 1: box runs past the client's row length", boxes=_tables(e, [[[2, 1, 3, 0], [2, 1, 2, 1]]], r)[1])
    bad("entry 0, client 1: box runs past the client's row length", boxes=_tables(e, [[[2, 1, 3, 0], [2, 1, 3, 0]]], r)[1])
    bad("entry 0, client 0: box runs past the client's row length", boxes=_tables(e, [[[2, 1, 3, 7], [2, 1, 2, 0]]], r)[1])
    bad("entry 0, client 1: box runs past the client's row length", boxes=_tables(e, [[[2, 1, 3, 0], [0, 1, 0, 5]]], r)[1])
    bad("entry 0, client 1: box runs past the client's row length", boxes=_tables(e, [[[2, 1, 3, 0], [2, 1, 2, -2]]], r)[1])
    bad("entry 0, client 1: an absent box has extents", boxes=_tables(e, [[[2, 1, 3, 0], [2, 1, 2, -1]]], r)[1])
    # an entry without elements and absent boxes only: accepted, and nothing to launch
    call(entries=_tables([[0, 0, 1, 3, 0, 0]], b, r)[0], boxes=_tables(e, [[[0, 0, 0, -1], [0, 1, 3, 4]]], r)[1])


def test_constants_match_the_header():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "plato_agg.h")).read()
    for name in ("MAX_K", "TILE", "ENTRY_WORDS", "BOX_WORDS"):
        value = getattr(_lib, "PLATO_AGG_SUBMODEL_" + name)
        assert f"#define PLATO_AGG_SUBMODEL_{name} {value}\n" in text
    assert "#define PLATO_AGG_SUBMODEL_ABSENT (-1)\n" in text and _lib.PLATO_AGG_SUBMODEL_ABSENT == -1
    assert sm.MAX_K == 4096 != _lib.PLATO_AGG_ROBUST_MAX_K
    assert isinstance(sm.compact_layout((("a.weight", (2, 3)),)), ArenaLayout)
