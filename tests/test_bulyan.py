"""Bulyan and Trimmed-mean on the CPU: the numpy restatements (tests/nearest_oracle.py) against the
reference fixtures, the host selection (plato_amd.krum.bulyan_select) on hand-made matrices, the
host-side argument checks of the nearest-mean mode of plato_agg_robust_columns, and the dispatch of
DetectorAggregationMixin (engine = test double).

The device side of the same cases is tests/test_bulyan_gpu.py.
"""

import asyncio
import os
import types

import numpy as np
import pytest

from plato_amd import _lib
from plato_amd.krum import bulyan_min_clients, bulyan_select
from tests import bulyan_cases as bc
from tests import krum_oracle as ko
from tests import nearest_oracle as no

CASES = bc.load_cases()
NAN = float("nan")


@pytest.fixture(scope="module")
def full():
    return bc.load_full()


def rows_of(case, k):
    return case["expected"]["selection"] if case["recipe"]["kind"] == "Bulyan" else list(range(k))


def check_values_against_fixture(case, got_f, got_i, xf, xi, full=None):
    """Off the listed boundary-tie columns: |got - ref| <= 2(b-1) 2^-24 sum|kept| / b per compared
    coordinate (the any-order summation bound over the kept values).  On them: the restatement, bit for
    bit.  Returns the number of coordinates compared with the reference."""
    recipe = case["recipe"]
    rows, trim = rows_of(case, xf.shape[0]), bc.trim_of(recipe)
    cols = {"f32": xf[rows], "i64": xi[rows].astype(np.float32)}
    got = {"f32": got_f, "i64": got_i}
    ties = {"f32": np.asarray(recipe["tie_f32"], dtype=np.int64), "i64": np.asarray(recipe["tie_i64"], dtype=np.int64)}
    checked = 0
    for region, idx, ref in bc.reference_values(case, full):
        x = cols[region][:, idx]
        listed = np.isin(idx, ties[region])
        bound = no.value_bound(x, trim)
        err = np.abs(got[region][idx].astype(np.float64) - ref.astype(np.float64))
        assert np.all(err[~listed] <= bound[~listed]), (region, int(np.argmax(err - bound)), float(np.max(err - bound)))
        if listed.any():
            exp = no.nearest_mean_columns(x[:, listed], trim)
            assert bc.canon(got[region][idx][listed]).tobytes() == bc.canon(exp).tobytes()
        checked += int((~listed).sum())
    assert checked >= 56
    return checked


def test_fixture_set_is_the_one_the_generator_writes(full):
    by_kind = lambda kind, model: [c["recipe"] for c in CASES  # noqa: E731
                                   if c["recipe"]["kind"] == kind and c["recipe"]["model"] == model]
    assert [(r["k"], r["f"]) for r in by_kind("Bulyan", "lenet5")] == list(bc.BULYAN_LENET)
    assert [(r["k"], r["f"]) for r in by_kind("Bulyan", "resnet18")] == list(bc.BULYAN_RESNET)
    assert [r["k"] for r in by_kind("Trimmed-mean", "lenet5")] == list(bc.TRIMMED_LENET)
    assert [r["k"] for r in by_kind("Trimmed-mean", "resnet18")] == list(bc.TRIMMED_RESNET)
    assert sorted(full.files) == sorted(n + ".f32" for n in bc.FULL)
    for c in CASES:
        r, e = c["recipe"], c["expected"]
        assert e["dtypes"] == ["torch.float32"]  # the counters too
        if r["kind"] == "Bulyan":
            theta = no.bulyan_theta(r["k"], r["f"])
            assert len(e["selection"]) == theta == len(set(e["selection"])) and theta - 2 * r["f"] >= 1
            assert e["selection"] != list(range(theta))  # the shuffle did its work
            d = 61706 if r["model"] == "lenet5" else None
            assert r["min_gap"] > r["required_gap"] == (2 * d * 2.0 ** -24 if d else 0.05)
        else:
            assert e["selection"] == [] and r["f"] == 0
        if r["model"] == "lenet5":
            assert len(r["tie_f32"]) + len(r["tie_i64"]) <= bc.MAX_TIES_LENET
        else:
            assert not set(r["tie_f32"]) & {j for j, _ in e["samples_f32"]}
            assert not set(r["tie_i64"]) & {j for j, _ in e["samples_i64f"]}


@pytest.mark.parametrize("case", CASES, ids=[c["recipe"]["name"] for c in CASES])
def test_restatement_equals_the_reference(case, full):
    recipe = case["recipe"]
    layout, xf, xi = bc.build_inputs(recipe)
    if recipe["kind"] == "Bulyan":
        dist = ko.pairwise_sqdist(xf, xi)
        sel = no.bulyan_select(dist, recipe["f"])
        assert sel == case["expected"]["selection"]  # exactly and in order
        assert bulyan_select(dist, recipe["f"]) == sel
    else:
        sel = list(range(recipe["k"]))
    trim = bc.trim_of(recipe)
    # full size: the stored samples and 8,192 more coordinates (every counter); else every coordinate
    at = np.arange(layout.n_f32) if recipe["model"] == "lenet5" else np.unique(np.concatenate(
        [bc.sample_index(layout.n_f32), np.random.default_rng(6).integers(0, layout.n_f32, 8192)]))
    sub_f, sub_i = xf[sel][:, at], xi[sel]
    got_f = np.full(layout.n_f32, np.nan, dtype=np.float32)
    got_f[at], got_i = no.nearest_mean(sub_f, sub_i, trim)
    check_values_against_fixture(case, got_f, got_i, xf, xi, full)
    # the boundary-tie columns, recomputed: none that the generator did not record
    tf = at[no.boundary_tie_columns(sub_f, trim)]
    ti = no.boundary_tie_columns(sub_i, trim) if sub_i.size else np.zeros(0, dtype=np.int64)
    assert set(tf.tolist()) <= set(recipe["tie_f32"]) and set(ti.tolist()) <= set(recipe["tie_i64"])
    if trim == 0:  # every row kept, in table order: the sequential mean
        exp_f, exp_i = ko.mean_rows(sub_f, sub_i, range(len(sel)))
        assert bc.canon(got_f[at]).tobytes() == bc.canon(exp_f).tobytes()
        assert bc.canon(got_i).tobytes() == bc.canon(exp_i).tobytes()


# ------------------------------------------------------------------ the restatement's own rules
def test_restatement_keeps_the_lowest_table_positions_among_equal_distances():
    x = np.array([[3.0], [1.0], [2.0], [2.0], [5.0], [-1.0]], dtype=np.float32)  # lower median 2; distances 1 1 0 0 3 3
    assert no.kept_rows(x, 1)[:, 0].tolist() == [True, True, True, True, False, False]
    assert no.nearest_mean_columns(x, 1)[0] == np.float32(2.0)
    assert no.kept_rows(x, 2)[:, 0].tolist() == [False, False, True, True, False, False]
    y = x[[1, 0, 2, 3, 5, 4]]  # 1 3 2 2 -1 5: b = 3 keeps the two 2s and the first of (1, 3) in the table
    assert no.kept_rows(y[:5], 1)[:, 0].tolist() == [True, False, True, True, False]
    assert no.boundary_tie_columns(y[:5], 1).tolist() == [0]
    assert no.boundary_tie_columns(x, 1).tolist() == [] and no.boundary_tie_columns(x, 0).tolist() == []
    inf = np.float32(np.inf)
    z = np.array([[inf], [inf], [1.0], [inf], [-inf]], dtype=np.float32)  # median +inf: NaN distances after +inf
    assert no.distance_keys(z)[:, 0].tolist() == [0x7FC00000] * 2 + [0x7F800000, 0x7FC00000, 0x7F800000]
    assert no.kept_rows(z, 1)[:, 0].tolist() == [True, False, True, False, True]
    assert np.isnan(no.nearest_mean_columns(z, 1)[0])  # inf + 1 + -inf
    n = np.array([[1.0], [np.nan], [2.0]], dtype=np.float32)
    assert no.nearest_mean_columns(n, 1).view(np.uint32)[0] == 0x7FC00000
    big = np.array([[(1 << 24) + 1], [(1 << 24) + 3], [0]], dtype=np.int64)
    assert no.nearest_mean_columns(big, 1)[0] == np.float32(1 << 24)  # 2^24 + 1 rounds to even; the median itself


# ------------------------------------------------------------------ the host selection
def _dist(points):
    p = np.asarray(points, dtype=np.float64)
    return (p[:, None] - p[None, :]) ** 2


def test_select_matches_the_naive_restatement_on_random_matrices():
    rng = np.random.default_rng(4)
    for k, f in ((6, 1), (9, 2), (13, 3), (16, 3), (20, 0), (33, 3), (64, 5), (129, 20), (256, 63)):
        x = rng.standard_normal((k, 5))
        d = ((x[:, None] - x[None]) ** 2).sum(-1)
        sel = bulyan_select(d, f)
        assert sel == no.bulyan_select(d, f) and len(sel) == min(k - 2 * f, k - 2 - f) == len(set(sel))


def test_select_breaks_ties_towards_the_lowest_index():
    # all clients identical: every score is 0 at every step
    assert bulyan_select(np.zeros((13, 13)), 3) == [0, 1, 2, 3, 4, 5, 6]
    # two mirror-image clusters: clients (0..4) and (5..9) have pairwise equal scores
    pts = [0.0, 1.0, 2.0, 3.0, 4.0, 24.0, 23.0, 22.0, 21.0, 20.0]
    sel = bulyan_select(_dist(pts), 2)
    assert sel == no.bulyan_select(_dist(pts), 2) and len(sel) == 6
    s = ko.scores_of(_dist(pts), list(range(10)), 2)
    tied = np.flatnonzero(s == s.min())
    assert tied.size > 1 and sel[0] == tied[0]
    # f <= 2: the last steps sum the diagonal's +0 alone and take the lowest remaining index
    pts = [9.0, 0.0, 0.5, 1.0, 1.75, 5.0]  # K = 6, f = 1: scores separate at m = 6, 5; one term at m = 4
    sel = bulyan_select(_dist(pts), 1)
    assert sel == no.bulyan_select(_dist(pts), 1)
    assert sel[2] == min(set(range(6)) - set(sel[:2]))


def test_select_ranks_nan_rows_last():
    pts = [0.0, 0.1, 0.25, 0.45, 0.7, 1.0, 1.35, 1.75, 2.2, 2.7, 3.3, 4.0, 4.8]
    d = _dist(pts)
    d[3, :] = d[:, 3] = NAN  # a NaN client: every distance to and from it (the kernel keeps the diagonal +0)
    d[3, 3] = 0.0
    sel = bulyan_select(d, 3)
    assert sel == no.bulyan_select(d, 3)
    assert 3 not in sel and len(sel) == 7
    # all scores NaN at the steps that sum two or more terms: the lowest index, every step
    assert bulyan_select(np.where(np.eye(13, dtype=bool), 0.0, NAN), 3) == list(range(7))


def test_select_refuses_every_k_f_that_leaves_nothing_to_average():
    for f in range(0, 7):
        need = bulyan_min_clients(f)
        assert need == max(4 * f + 1, 3 * f + 3)
        for k in range(1, need + 3):
            theta = min(k - 2 * f, k - 2 - f)
            if theta - 2 * f < 1:
                assert k < need
                with pytest.raises(ValueError, match=f"at least {need} clients, got {k}"):
                    bulyan_select(np.zeros((k, k)), f)
                with pytest.raises(ValueError):
                    no.bulyan_select(np.zeros((k, k)), f)
            else:
                assert k >= need and bulyan_select(np.zeros((k, k)), f) == list(range(theta))
    with pytest.raises(ValueError, match="square"):
        bulyan_select(np.zeros((7, 8)), 1)
    with pytest.raises(ValueError, match="f must be >= 0"):
        bulyan_select(np.zeros((7, 7)), -1)


# ------------------------------------------------------------------ host refusals of the C entry point
def test_mode_1_argument_errors_are_raised_without_gpu_work():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    assert _lib.PLATO_AGG_ROBUST == {"median": 0, "nearest_mean": 1}
    a = 1 << 12  # an aligned non-null address: nothing is dereferenced on these paths
    call = lambda *args: _lib.call("plato_agg_robust_columns", *args)  # noqa: E731
    # mode 1 is accepted: the refusals below are the checks behind the mode's
    with pytest.raises(ValueError, match="null"):
        call(1, None, None, 4, 1, a, None, 64, 0, None)
    with pytest.raises(ValueError, match="null int64"):
        call(1, a, None, 4, 0, a, a, 64, 1, None)
    with pytest.raises(ValueError, match="aligned"):
        call(1, a + 4, None, 4, 1, a, None, 64, 0, None)
    with pytest.raises(ValueError, match="aligned"):
        call(1, a, None, 4, 1, a + 4, None, 64, 0, None)
    for k, trim in ((4, 2), (4, -1), (1, 1), (5, 3), (256, 128)):
        with pytest.raises(ValueError, match="trim"):
            call(1, a, None, k, trim, a, None, 64, 0, None)
    for k in (0, 257):
        with pytest.raises(ValueError, match=r"K must be in 1\.\.256"):
            call(1, a, None, k, 0, a, None, 64, 0, None)
    for mode in (2, -1):
        with pytest.raises(ValueError, match="mode"):
            call(mode, a, None, 4, 0, a, None, 64, 0, None)
    call(1, None, None, 5, 2, None, None, 0, 0, None)  # nothing to do: no launch, no error
    assert _lib.ABI_VERSION == 5 and _lib.lib().plato_agg_abi_version() == 5


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

    from plato_amd.servers import DetectorAggregationMixin

    s = type("Server", (DetectorAggregationMixin,), {"secure_aggregation_type": kind, **attrs})()
    s._plato_amd_engine = _Engine()
    updates = [types.SimpleNamespace(report=types.SimpleNamespace(num_samples=n)) for n in (1, 3)]
    payloads = [{"w": torch.zeros(2)}, {"w": torch.ones(2)}]
    return s, updates, payloads


def _run(s, updates, payloads):
    return asyncio.run(s.aggregate_weights(updates, payloads[0], payloads))


def test_hook_bulyan_launches_with_the_configured_attackers_and_releases_arrivals(monkeypatch):
    from plato_amd.servers import robust

    s, updates, payloads = _server("Bulyan", num_attackers=3)
    monkeypatch.setattr(robust, "_num_attackers", lambda: pytest.fail("num_attackers is set: no Config read"))
    assert _run(s, updates, payloads) == {"w": 1}
    assert s._plato_amd_engine.log == ["client", "client", ("launch_bulyan", 3)]
    assert s._plato_amd_engine.released == 1
    # unset: len(Config().clients.attacker_ids), as the reference reads it
    s, updates, payloads = _server("Bulyan")
    monkeypatch.setattr(robust, "_num_attackers", lambda: 5)
    assert _run(s, updates, payloads) == {"w": 1}
    assert s._plato_amd_engine.log == ["client", "client", ("launch_bulyan", 5)]
    assert s._plato_amd_engine.released == 1


def test_hook_trimmed_mean_launches_the_nearest_mean_with_the_references_trim():
    s, updates, payloads = _server("Trimmed-mean")
    assert _run(s, updates, payloads) == {"w": 1}
    assert s._plato_amd_engine.log == ["client", "client", ("launch_robust", "nearest_mean", 0)]
    assert s._plato_amd_engine.released == 1
    s, updates, payloads = _server("Trimmed-mean", trim=1)
    _run(s, updates, payloads)
    assert s._plato_amd_engine.log[-1] == ("launch_robust", "nearest_mean", 1)


def test_hook_hands_every_other_name_to_the_parent():
    s, updates, payloads = _server("Median")
    assert _run(s, updates, payloads) == {"w": 1}
    assert s._plato_amd_engine.log == ["client", "client", ("launch_robust", "median", 0)]
    assert s._plato_amd_engine.released == 1
    s, updates, payloads = _server("Multi-krum")
    assert _run(s, updates, payloads) == {"w": 1}
    assert s._plato_amd_engine.log == ["client", "client", ("launch_multi_krum", 2)]
    assert s._plato_amd_engine.released == 1
    s, updates, payloads = _server(None)  # the reference's "Fedavg is applied" branch
    s.robust_aggregation_type = lambda: None
    assert _run(s, updates, payloads) == {"w": 1}
    assert s._plato_amd_engine.log[-1] == ("launch", [0.25, 0.75])


@pytest.mark.parametrize("name", ["Krum", "Afa", "Fl-trust", "bulyan", "Trimmed-Mean"])
def test_hook_refuses_unknown_names_without_touching_the_engine(name):
    s, updates, payloads = _server(name)
    with pytest.raises(ValueError, match="supported: Bulyan, Median, Multi-krum, Trimmed-mean"):
        _run(s, updates, payloads)
    assert s._plato_amd_engine.log == [] and s._plato_amd_engine.released == 0


@pytest.mark.parametrize("kind", ["Bulyan", "Trimmed-mean"])
def test_hook_refuses_several_aggregation_devices_before_staging(kind):
    s, updates, payloads = _server(kind, num_attackers=0)
    s._plato_amd_engine.primary = object()  # what a multi-GPU engine carries
    with pytest.raises(NotImplementedError, match="one GPU"):
        _run(s, updates, payloads)
    assert s._plato_amd_engine.log == [] and s._plato_amd_engine.released == 0


def test_hook_refuses_coded_payloads_before_any_engine_call():
    import torch

    for kind in ("Bulyan", "Trimmed-mean"):
        s, updates, payloads = _server(kind, num_attackers=0)
        coded = [{"w": torch.zeros(2, dtype=torch.bfloat16)}, {"w": torch.ones(2, dtype=torch.bfloat16)}]
        with pytest.raises(ValueError, match="native payloads"):
            _run(s, updates, coded)
        assert s._plato_amd_engine.log == []
