"""Multi-Krum on the CPU: the numpy restatements against the reference fixtures, the host selection
(plato_amd.krum) on hand-made matrices, the host-side argument checks of the three C entry points, and
the hook's dispatch (engine = test double).

The device side of the same cases is tests/test_krum_gpu.py.
"""

import asyncio
import os
import types

import numpy as np
import pytest

from plato_amd import _lib
from plato_amd.krum import multi_krum_select
from tests import krum_cases as kc
from tests import krum_oracle as ko

CASES = kc.load_cases()
NAN = float("nan")


@pytest.fixture(scope="module")
def full():
    return kc.load_full()


def check_mean_against_fixture(case, got_f, got_i, xf, xi, full=None):
    """|got - ref| <= 2(m-1) 2^-24 sum_k|x_k| / m + 2 * 2^-24 |ref| + 2^-149 per compared coordinate, over
    the selected rows: the any-order summation bound on both sides plus the two divisions."""
    sel = case["expected"]["selection"]
    cols = {"f32": xf, "i64": xi.astype(np.float32)}
    got = {"f32": got_f, "i64": got_i}
    checked = 0
    for region, idx, ref in kc.reference_values(case, full):
        bound = ko.mean_bound(cols[region][:, idx], sel, ref)
        err = np.abs(got[region][idx].astype(np.float64) - ref.astype(np.float64))
        assert np.all(err <= bound), (region, int(np.argmax(err - bound)), float(np.max(err - bound)))
        checked += idx.size
    assert checked >= 56


def test_fixture_set_is_the_one_the_generator_writes(full):
    assert [c["recipe"]["k"] for c in CASES if c["recipe"]["model"] == "lenet5"] == list(kc.KS_LENET)
    assert [c["recipe"]["k"] for c in CASES if c["recipe"]["model"] == "resnet18"] == [8]
    assert sorted(full.files) == sorted(f"mkrum_lenet5_k{k}.f32" for k in kc.FULL_KS)
    for c in CASES:
        r, e = c["recipe"], c["expected"]
        assert e["dtypes"] == ["torch.float32"]  # the counters too
        assert len(e["selection"]) == r["k"] - 2 * r["f"] - 2 and len(set(e["selection"])) == len(e["selection"])
        assert e["selection"] != list(range(len(e["selection"])))  # the shuffle did its work
        d = 61706 if r["model"] == "lenet5" else None
        assert r["min_gap"] > r["required_gap"] == (2 * d * 2.0 ** -24 if d else 0.05)


@pytest.mark.parametrize("case", CASES, ids=[c["recipe"]["name"] for c in CASES])
def test_restatement_equals_the_reference(case, full):
    layout, xf, xi = kc.build_inputs(case["recipe"])
    dist = ko.pairwise_sqdist(xf, xi)
    sel = ko.select(dist, case["recipe"]["f"])
    assert sel == case["expected"]["selection"]  # exactly and in order
    assert multi_krum_select(dist, case["recipe"]["f"]) == sel
    got_f, got_i = ko.mean_rows(xf, xi, sel)
    check_mean_against_fixture(case, got_f, got_i, xf, xi, full)


# ------------------------------------------------------------------ the host selection
def _dist(points):
    p = np.asarray(points, dtype=np.float64)
    return (p[:, None] - p[None, :]) ** 2


def test_select_matches_the_naive_restatement_on_random_matrices():
    rng = np.random.default_rng(3)
    for k in (7, 8, 9, 20, 64, 129, 256):
        x = rng.standard_normal((k, 5))
        d = ((x[:, None] - x[None]) ** 2).sum(-1)
        assert multi_krum_select(d, 2) == ko.select(d, 2)
    d = ((x[:, None] - x[None]) ** 2).sum(-1)
    for f in (0, 1, 5):
        assert multi_krum_select(d, f) == ko.select(d, f)


def test_select_breaks_ties_towards_the_lowest_index():
    # all clients identical: every score is 0 at every step
    assert multi_krum_select(np.zeros((9, 9)), 2) == [0, 1, 2]
    # two mirror-image clusters: clients (0, 1, 2, 3) and (4, 5, 6, 7) have pairwise equal scores
    pts = [0.0, 1.0, 2.0, 3.0, 13.0, 12.0, 11.0, 10.0]
    sel = multi_krum_select(_dist(pts), 2)
    assert sel == ko.select(_dist(pts), 2) and len(sel) == 2
    s = ko.scores_of(_dist(pts), list(range(8)), 2)
    tied = np.flatnonzero(s == s.min())
    assert tied.size > 1 and sel[0] == tied[0]


def test_select_ranks_nan_rows_last():
    pts = [0.0, 0.1, 0.25, 0.45, 0.7, 1.0, 1.35, 1.75, 2.2]
    d = _dist(pts)
    d[3, :] = d[:, 3] = NAN  # a NaN client: every distance to and from it (the kernel keeps the diagonal +0)
    d[3, 3] = 0.0
    sel = multi_krum_select(d, 2)
    assert sel == ko.select(d, 2)
    assert 3 not in sel and len(sel) == 3
    # NaN sorts last inside a row: the other clients' scores stay finite while enough finite distances remain
    assert np.isfinite(ko.scores_of(d, list(range(9)), 2)[[0, 1, 2, 4]]).all()
    # all scores NaN: the lowest index, every step
    assert multi_krum_select(np.where(np.eye(7, dtype=bool), 0.0, NAN), 2) == [0]


def test_select_refuses_too_few_clients_and_takes_the_smallest_k():
    for k in (1, 5, 6):  # K <= 2f + 2
        with pytest.raises(ValueError, match="more than 6 clients"):
            multi_krum_select(np.zeros((k, k)), 2)
    with pytest.raises(ValueError, match="more than 2 clients"):
        multi_krum_select(np.zeros((2, 2)), 0)
    with pytest.raises(ValueError, match="square"):
        multi_krum_select(np.zeros((7, 8)), 2)
    pts = [5.0, 0.0, 0.5, 1.0, 1.75, 9.0, 0.25]  # K = 2f + 3: one step, one pick
    sel = multi_krum_select(_dist(pts), 2)
    assert sel == ko.select(_dist(pts), 2) == [6]  # sum of the 3 smallest of its row: 0 + 1/16 + 1/16


# ------------------------------------------------------------------ host refusals of the C entry points
def test_argument_errors_are_raised_without_gpu_work():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    a = 1 << 12  # an aligned non-null address: nothing is dereferenced on these paths
    dist = lambda *args: _lib.call("plato_agg_pairwise_sqdist", *args)  # noqa: E731
    for k in (0, 257):
        with pytest.raises(ValueError, match=r"K must be in 1\.\.256"):
            dist(a, None, k, 64, 0, a, a, None)
    with pytest.raises(ValueError, match="null fp32"):
        dist(None, None, 4, 64, 0, a, a, None)
    with pytest.raises(ValueError, match="null int64"):
        dist(a, None, 4, 64, 1, a, a, None)
    with pytest.raises(ValueError, match="null output or workspace"):
        dist(a, None, 4, 64, 0, None, a, None)
    with pytest.raises(ValueError, match="null output or workspace"):
        dist(a, None, 4, 64, 0, a, None, None)
    with pytest.raises(ValueError, match="tables must be 8-byte aligned"):
        dist(a + 4, None, 4, 64, 0, a, a, None)
    with pytest.raises(ValueError, match="matrix must be 16-byte aligned"):
        dist(a, None, 4, 64, 0, a, a + 8, None)
    with pytest.raises(ValueError, match="workspace must be 256-byte aligned"):
        dist(a, None, 4, 64, 0, a + 128, a, None)
    with pytest.raises(ValueError, match="coordinates"):
        dist(a, None, 4, 1 << 38, 0, a, a, None)
    ws = _lib.lib().plato_agg_pairwise_sqdist_workspace
    assert ws(0, 64, 0) == 0 and ws(257, 64, 0) == 0 and ws(4, 1 << 38, 0) == 0
    assert ws(1, 1, 0) == 8192 and ws(32, 1, 1) == 2 * 8192 and ws(33, 1, 0) == 3 * 8192  # chunks x tiles x 32 x 32 x 8
    assert ws(256, 11_181_642, 0) % 256 == 0 and 0 < ws(256, 11_181_642, 0) <= 256 * 36 * 8192
    assert ws(4, 0, 0) == 256

    mean = lambda *args: _lib.call("plato_agg_mean_rows", *args)  # noqa: E731
    for m in (0, 257):
        with pytest.raises(ValueError, match=r"m must be in 1\.\.256"):
            mean(a, None, m, a, None, 64, 0, None)
    with pytest.raises(ValueError, match="null fp32"):
        mean(a, None, 4, None, None, 64, 0, None)
    with pytest.raises(ValueError, match="null int64"):
        mean(a, a, 4, a, None, 64, 1, None)
    with pytest.raises(ValueError, match="aligned"):
        mean(a + 4, None, 4, a, None, 64, 0, None)
    with pytest.raises(ValueError, match="aligned"):
        mean(a, None, 4, a + 4, None, 64, 0, None)
    with pytest.raises(ValueError, match="coordinates"):
        mean(a, None, 4, a, None, 1 << 38, 0, None)
    assert _lib.ABI_VERSION == 5 and _lib.lib().plato_agg_abi_version() == 5
    assert _lib.PLATO_AGG_PAIRDIST_CHAIN == header_constant("PLATO_AGG_PAIRDIST_CHAIN")


def header_constant(name: str) -> int:
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(os.path.dirname(here), "include", "plato_agg.h")) as f:
        for line in f:
            parts = line.split()
            if len(parts) >= 3 and parts[0] == "#define" and parts[1] == name:
                return int(parts[2])
    raise KeyError(name)


def test_a_stale_library_asks_for_a_rebuild():
    handle = types.SimpleNamespace(_name="libplato_agg.so")  # no symbol at all
    with pytest.raises(RuntimeError, match="lacks plato_agg_mean_rows; rebuild it"):
        _lib._bind(handle, {"plato_agg_mean_rows": _lib.SIGNATURES["plato_agg_mean_rows"]})


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

    def launch_multi_krum(self, f=2, order=None):
        self.log.append(("launch_multi_krum", f))

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


def test_hook_multi_krum_launches_with_the_references_f_and_releases_arrivals():
    s, updates, payloads = _server("Multi-krum")
    assert asyncio.run(s.aggregate_weights(updates, payloads[0], payloads)) == {"w": 1}
    assert s._plato_amd_engine.log == ["client", "client", ("launch_multi_krum", 2)]
    assert s._plato_amd_engine.released == 1


@pytest.mark.parametrize("name", ["Krum", "Bulyan", "multi-krum", "krum"])
def test_hook_refusal_lists_both_supported_names(name):
    s, updates, payloads = _server(name)
    with pytest.raises(ValueError, match="supported: Median, Multi-krum"):
        asyncio.run(s.aggregate_weights(updates, payloads[0], payloads))
    assert s._plato_amd_engine.log == []
