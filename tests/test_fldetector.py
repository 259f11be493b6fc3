"""FLDetector without a GPU: the numpy restatement (tests/fldetector_oracle.py) and the host scalars
(plato_amd.detectors) against the reference fixtures (tests/golden/fldetector_*), the exact 2-means split
against brute force, the record's checkpoints and arena order, the server hook's dispatch and refusals on
stubs, and the host-side argument checks of the four kernels.

Bound against the reference (from its own error, never from the code under test): started from the
reference's record, the distances of a round are within ``ref_err`` of ``exact``, where ``exact`` is the
float64 evaluation of the reference's formula on its own fp32 inputs and ``ref_err`` the reference's own
relative distance from it (both figures of the fixture; cond(mat) < 1e6 there, so ``exact`` is exact to
about 1e-10).
"""

import functools
import itertools
import os
import types

import numpy as np
import pytest

from plato_amd import _lib
from plato_amd import detectors as host
from tests import fldetector_cases as fc
from tests import fldetector_oracle as fo

CASES = fc.load_cases()
NAMES = [c["recipe"]["name"] for c in CASES]
ROUNDS = [(c["recipe"]["name"], t) for c in CASES for t in range(1, c["recipe"]["rounds"])]


def case_of(name):
    return next(c for c in CASES if c["recipe"]["name"] == name)


@functools.lru_cache(maxsize=None)
def full_arrays():
    return fc.load_full()


@functools.lru_cache(maxsize=None)
def layout_index(name):
    lay = fc.layout_of(case_of(name)["recipe"])
    return lay, host.arena_index(lay)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


# ------------------------------------------------------------------ the restatement against the reference
def test_the_recipes_are_the_fixtures():
    assert [c["recipe"] for c in CASES] == fc.recipes()
    assert {c["recipe"]["k"] for c in CASES} == {3, 8, 9}
    assert {len(c["recipe"]["attackers"]) for c in CASES} == {0, 1, 2}
    assert any(layout_index(n)[0].n_i64 for n in NAMES) and not all(layout_index(n)[0].n_i64 for n in NAMES)
    for c in CASES:
        assert all(r["cond"] < 1e6 for r in c["rounds"][1:])
        assert all(r["gap_over_range"] >= 0.25 for r in c["rounds"][1:])


@pytest.mark.parametrize("name,t", ROUNDS)
def test_restatement_from_the_references_record_is_within_its_own_error(name, t):
    case = case_of(name)
    lay, index = layout_index(name)
    rec = fo.Record.from_reference(*fc.reference_record(case, full_arrays(), t, lay), index)
    bf, bi, xf, xi, ids = fc.scenario(name)[t]
    got = rec.round(xf, xi, bf, bi, ids)
    expected = case["rounds"][t]
    exact = fc.f64s(expected["exact"])
    err = float(np.max(np.abs(np.sqrt(got["d2"]) - exact) / exact))
    print(f"{name} round {t}: err {err:.3e}, ref_err {expected['ref_err']:.3e}, cond {got['cond']:.3e}")
    assert err <= expected["ref_err"]
    assert got["malicious"] == sorted(expected["malicious"])


@pytest.mark.parametrize("name", NAMES)
def test_a_whole_scenario_on_the_restatements_own_record_flags_what_the_reference_flags(name):
    case = case_of(name)
    lay, index = layout_index(name)
    rec = fo.Record(index.size)
    worst = 0.0
    for t, (bf, bi, xf, xi, ids) in enumerate(fc.scenario(name)):
        got = rec.round(xf, xi, bf, bi, ids)
        expected = case["rounds"][t]
        assert ids == expected["ids"] and got["malicious"] == sorted(expected["malicious"]), t
        if t:
            ref = fc.hexes(expected["normalised"]).astype(np.float64)
            worst = max(worst, float(np.max(np.abs(got["distances"].astype(np.float64) - ref))))
        # the cache grown row by row holds what a recompute from the rows gives
        sy, ss, yy = rec.full_gram()
        assert np.array_equal(bits(sy), bits(rec.sy)) and np.array_equal(bits(ss), bits(rec.ss))
        assert np.array_equal(bits(yy), bits(rec.yy))
        assert np.array_equal(bits(rec.ss), bits(rec.ss.T))
    print(f"{name}: max |normalised distance - reference's| over the scenario {worst:.3e}")
    assert case["rounds"][0]["malicious"] == [] and case["rounds"][0]["distances"] is None


def test_round_zero_starts_the_record_with_the_baseline_and_the_mean():
    name = NAMES[0]
    bf, bi, xf, xi, ids = fc.scenario(name)[0]
    rec = fo.Record(layout_index(name)[1].size)
    got = rec.round(xf, xi, bf, bi, ids)
    assert got["malicious"] == [] and got["scores"] is None
    assert np.array_equal(bits(rec.s[0]), bits(fo.flat(bf, bi)))
    assert np.array_equal(bits(rec.y[0]), bits(got["g"]))
    assert all(rec.history[c] == [None] for c in ids)


# ------------------------------------------------------------------ the exact 2-means split
def brute_force(scores):
    """The least within-cluster sum of squares over every split into two non-empty sets."""
    x = np.asarray(scores, dtype=np.float64)
    best = np.inf
    for r in range(1, len(x)):
        for hi in itertools.combinations(range(len(x)), r):
            mask = np.zeros(len(x), dtype=bool)
            mask[list(hi)] = True
            a, b = x[mask], x[~mask]
            best = min(best, float(np.sum((a - a.mean()) ** 2) + np.sum((b - b.mean()) ** 2)))
    return best


def cost_of(scores, flagged):
    x = np.asarray(scores, dtype=np.float64)
    mask = np.zeros(len(x), dtype=bool)
    mask[flagged] = True
    a, b = x[mask], x[~mask]
    return float(np.sum((a - a.mean()) ** 2) + np.sum((b - b.mean()) ** 2))


SCORE_SETS = [[0.1, 0.9], [0.9, 0.1], [0.1, 0.11, 0.9], [0.5, 0.1, 0.45, 0.12], [0.3, 0.1, 0.2, 0.9, 0.95],
              [0.1, 0.2, 0.3, 0.4, 0.5, 0.6], [0.11, 0.1, 0.1, 0.3, 0.3, 0.29], [1.0, 0.0, 0.0, 0.0, 0.0, 0.0],
              [0.2, 0.2, 0.7, 0.7], [0.25, 0.125, 0.5, 0.0625, 0.75, 0.375], [3.0, 1.0, 2.0], [0.1, 0.1, 0.1, 0.4]]


@pytest.mark.parametrize("scores", SCORE_SETS)
def test_two_means_is_the_brute_force_optimum(scores):
    flagged, clean = host.two_means_1d(np.float32(scores))
    assert sorted(flagged + clean) == list(range(len(scores))) and flagged and clean
    x = np.float32(scores).astype(np.float64)
    assert cost_of(x, flagged) == pytest.approx(brute_force(x), rel=1e-12, abs=1e-300)
    assert x[flagged].mean() > x[clean].mean()  # the lower-mean cluster is clean
    assert x[flagged].min() > x[clean].max()    # and the clusters are contiguous


def test_two_means_rules_for_ties_two_clients_and_equal_scores():
    assert host.two_means_1d([0.2, 0.7]) == ([1], [0]) and host.two_means_1d([0.7, 0.2]) == ([0], [1])
    # equal scores are never separated
    assert host.two_means_1d([0.5, 0.1, 0.5, 0.1]) == ([0, 2], [1, 3])
    # two splits of equal cost: the one that flags fewer clients
    assert host.two_means_1d([0.0, 1.0, 2.0]) == ([2], [0, 1])
    assert host.two_means_1d([2.0, 0.0, 4.0, 6.0]) == ([2, 3], [0, 1])  # cost 4; flagging 6 alone costs 8
    # all equal, and one client: one cluster, nobody is flagged
    assert host.two_means_1d([0.25] * 5) == ([], [0, 1, 2, 3, 4])
    assert host.two_means_1d([0.25]) == ([], [0])
    for bad in ([0.1, np.nan], [np.inf, 0.1]):
        with pytest.raises(ValueError, match="non-finite"):
            host.two_means_1d(bad)


# ------------------------------------------------------------------ the host scalars
def test_history_score_is_the_references_fp32_running_mean():
    past = [None, np.float32(0.1), np.float32(0.2), None]
    now = np.float32(0.3)
    scores = [v for v in past if v is not None]
    scores.append(now)
    assert bits(host.history_score(past, now)) == bits(np.float32(sum(scores) / len(scores)))
    assert bits(host.history_score([None], now)) == bits(now)


def test_a_singular_or_non_finite_system_and_a_nan_score_raise():
    one = np.ones((1, 1))
    with pytest.raises(ValueError, match="not finite"):  # y_last = 0: two identical rounds
        host.lbfgs_coefficients(one, one, 0.0, np.ones(1), np.ones(1))
    with pytest.raises(ValueError, match="not finite"):
        host.lbfgs_coefficients(one * np.nan, one, 1.0, np.ones(1), np.ones(1))
    with pytest.raises(ValueError, match="singular"):  # s . y = 0: a zero diagonal block and a zero S S^T
        host.lbfgs_coefficients(np.zeros((1, 1)), one, 1.0, np.ones(1), np.ones(1))
    for d2 in ([1.0, np.nan], [np.inf, 1.0], [0.0, 0.0], [-1.0, 1.0]):
        with pytest.raises(ValueError, match="non-finite or all-zero"):
            host.normalised_distances(d2)
    out = host.normalised_distances([4.0, 1e300, 0.0])  # the root is taken in float64: no overflow
    assert out.dtype == np.float32 and np.all(np.isfinite(out))


def test_lbfgs_coefficients_solve_the_references_system():
    rng = np.random.default_rng(5)
    s, y = rng.standard_normal((3, 40)), rng.standard_normal((3, 40))
    y = s * 0.8 + 0.05 * y
    v = rng.standard_normal(40)
    sy, ss = s @ y.T, s @ s.T
    got = host.lbfgs_coefficients(sy, ss, float(y[-1] @ y[-1]), s @ v, y @ v)
    sigma = sy[-1, -1] / (y[-1] @ y[-1])
    low = sy - np.triu(sy)
    mat = np.block([[sigma * ss, low], [low.T, -np.diag(np.diag(sy))]])
    hvp = sigma * v - np.concatenate([sigma * s.T, y.T], axis=1) @ np.linalg.inv(mat) @ np.concatenate(
        [s @ (sigma * v), y @ v])
    mine = sigma * v - np.concatenate([s, y]).T @ got["a"]
    assert got["sigma"] == sigma and np.allclose(mine, hvp, rtol=1e-9, atol=1e-12)
    assert got["cond"] == pytest.approx(np.linalg.cond(mat))


# ------------------------------------------------------------------ the record: arena order and checkpoints
def test_arena_index_moves_the_counters_behind_the_fp32_entries():
    lay, index = layout_index("fld_bn_k8_a2")
    assert lay.n_i64 == 5 and sorted(index) == list(range(lay.n_f32 + lay.n_i64))
    flat = np.arange(index.size, dtype=np.float32)  # state-dict order
    row = host._flat_host(flat, index).numpy()
    at = 0
    for e in lay.entries:
        lo = e.offset if e.region == "f32" else lay.n_f32 + e.offset
        assert np.array_equal(row[lo:lo + e.numel], flat[at:at + e.numel])
        at += e.numel
    assert np.array_equal(row[lay.n_f32:], flat[[e_at for e_at in _counter_positions(lay)]])
    from plato_amd.arena import ArenaLayout, Entry

    padded = ArenaLayout([Entry("a", "f32", 0, 3, (3,)), Entry("b", "f32", 4, 5, (5,))], 9, 0)
    with pytest.raises(ValueError, match="no alignment padding"):
        host.arena_index(padded)


def _counter_positions(lay):
    at, out = 0, []
    for e in lay.entries:
        if e.region == "i64":
            out.extend(range(at, at + e.numel))
        at += e.numel
    return out


def test_the_references_record_round_trips_through_the_checkpoint():
    name, t = "fld_bn_k8_a2", 4
    case = case_of(name)
    lay, index = layout_index(name)
    s, y, last_w, last_g, scores = fc.reference_record(case, full_arrays(), t, lay)
    state = host.FLDetectorState()
    state.load_reference_record(s, y, last_w, last_g, scores, lay)
    assert len(state) == t and state.dim == index.size and state.device is None
    exp = fo.Record.from_reference(s, y, last_w, last_g, scores, index)
    for got, want in zip(state.s_rows + state.y_rows + [state.last_w, state.last_g],
                         exp.s + exp.y + [exp.last_w, exp.last_g]):
        assert np.array_equal(bits(got.numpy()), bits(want))
    saved = state.state_dict()
    assert saved["gram"] is None and saved["S"].shape == (t, index.size)
    again = host.FLDetectorState()
    again.load_state_dict(saved)
    back = again.state_dict()
    for key in ("S", "Y", "last_w", "last_g"):
        assert np.array_equal(bits(back[key].numpy()), bits(saved[key].numpy())), key
    assert back["history"] == saved["history"] == {k: list(v) for k, v in scores.items()}
    assert back["signature"] == lay.signature and back["rounds"] == t and back["gram"] is None
    # a window keeps the newest rows only
    windowed = host.FLDetectorState(max_records=2)
    windowed.load_reference_record(s, y, last_w, last_g, scores, lay)
    assert len(windowed) == 2 and np.array_equal(bits(windowed.s_rows[0].numpy()), bits(exp.s[t - 2]))
    with pytest.raises(ValueError, match="max_records"):
        host.FLDetectorState(max_records=0)
    with pytest.raises(ValueError, match="as many"):
        state.load_reference_record(s, y[:-1], last_w, last_g, scores, lay)
    with pytest.raises(ValueError, match="elements"):
        state.load_reference_record([r[:-1] for r in s], y, last_w, last_g, scores, lay)


# ------------------------------------------------------------------ the server hook (stubs)
class _Base:
    base_calls = 0

    def weights_filter(self, weights_attacked):
        self.base_calls += 1
        return "base"


class _Engine:
    def __init__(self):
        self.log = []

    def begin(self, template, k, codec="native"):
        self.log.append(("begin", k))
        raise AssertionError("the refusals come before any engine call")


def _server(detector_type):
    import torch

    from plato_amd.servers import DetectorFilterMixin, TrustAggregationMixin, AttackSimulationMixin

    mixin = type("Mixin", (DetectorFilterMixin, AttackSimulationMixin, TrustAggregationMixin), {})
    server = type("Server", (mixin, _Base), {"detector_type": detector_type})()
    server._plato_amd_engine = _Engine()
    server.updates = [types.SimpleNamespace(client_id=i + 1) for i in range(2)]
    server.algorithm = types.SimpleNamespace(extract_weights=lambda: {"w": torch.zeros(2)})
    return server, [{"w": torch.zeros(2)}, {"w": torch.ones(2)}]


@pytest.mark.parametrize("name", ["AsyncFilter", "fldetector", "Krum"])
def test_hook_sends_every_other_detector_to_the_base_class(name):
    server, payloads = _server(name)
    assert server.weights_filter(payloads) == "base" and server.base_calls == 1
    assert server._plato_amd_engine.log == []


def test_hook_sends_an_absent_detector_type_to_the_base_class(monkeypatch):
    from plato_amd.servers import robust

    server, payloads = _server(None)
    monkeypatch.setattr(robust, "_detector_type", lambda: None)
    assert server.weights_filter(payloads) == "base" and server.base_calls == 1
    monkeypatch.setattr(robust, "_detector_type", lambda: "AsyncFilter")
    assert server.weights_filter(payloads) == "base" and server.base_calls == 2


def test_hook_refuses_codes_several_devices_and_too_many_clients_before_any_engine_call():
    import torch

    server, payloads = _server("FLDetector")
    coded = [{"w": torch.zeros(2, dtype=torch.bfloat16)}, {"w": torch.ones(2, dtype=torch.bfloat16)}]
    with pytest.raises(ValueError, match="native payloads"):
        server.weights_filter(coded)
    server._plato_amd_engine.primary = object()  # what a multi-GPU engine carries
    with pytest.raises(NotImplementedError, match="one GPU"):
        server.weights_filter(payloads)
    del server._plato_amd_engine.primary
    many = [payloads[0]] * (_lib.PLATO_AGG_ROBUST_MAX_K + 1)
    with pytest.raises(ValueError, match="at most 256 clients"):
        server.weights_filter(many)
    assert server._plato_amd_engine.log == [] and server.base_calls == 0
    from plato_amd.multi import MultiRound

    with pytest.raises(NotImplementedError, match="one GPU"):
        MultiRound.launch_fldetector(object(), [1])


# ------------------------------------------------------------------ ABI
def test_detect_argument_errors_are_raised_without_gpu_work():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = _lib.lib()
    a = 1 << 12  # an aligned non-null address: nothing is dereferenced on these paths
    assert _lib.ABI_VERSION == 5 and lib.plato_agg_abi_version() == 5
    for name in ("plato_agg_detect_means", "plato_agg_rows_dots", "plato_agg_rows_dots_workspace",
                 "plato_agg_lbfgs_predict", "plato_agg_delta_sqdist", "plato_agg_delta_sqdist_workspace"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    tile = _lib.PLATO_AGG_TRUST_TILE
    ws = lib.plato_agg_rows_dots_workspace
    assert ws(0, 1, 64) == 0 and ws(65537, 1, 64) == 0 and ws(4, 0, 64) == 0 and ws(4, 5, 64) == 0
    assert ws(4, 3, 1 << 38) == 0 and ws(4, 3, 0) == 256
    assert ws(4, 3, 1) == 12 * 8 and ws(5, 4, tile + 1) == 2 * 20 * 8 and ws(1, 1, 1024 * tile + 1) == 513 * 8
    ws = lib.plato_agg_delta_sqdist_workspace
    assert ws(0, 64, 0) == 0 and ws(257, 64, 0) == 0 and ws(4, 1 << 38, 0) == 0 and ws(4, 0, 1 << 38) == 0
    assert ws(4, 0, 0) == 256 and ws(4, 1, 0) == 4 * 8 and ws(9, tile + 1, 3) == 3 * 9 * 8

    # detect_means: (x_f32, x_i64, K, b_f32, b_i64, last_w, last_g, g, v, s_new, y_new, b_flat, n_f32, n_i64, stream)
    means = lambda *args: _lib.call("plato_agg_detect_means", *args, None)  # noqa: E731
    for k in (0, 257, -3):
        with pytest.raises(ValueError, match=r"K must be in 1\.\.256"):
            means(a, None, k, a, None, a, a, a, a, a, a, a, 64, 0)
    for args in ((None, None, 4, a, None, a, a, a, a, a, a, a, 64, 0), (a, None, 4, None, None, a, a, a, a, a, a, a, 64, 0)):
        with pytest.raises(ValueError, match="null fp32"):
            means(*args)
    with pytest.raises(ValueError, match="null int64"):
        means(a, None, 4, a, a, a, a, a, a, a, a, a, 64, 1)
    for hole in range(5, 12):
        args = [a, None, 4, a, None, a, a, a, a, a, a, a, 64, 0]
        args[hole] = None
        with pytest.raises(ValueError, match="null flat row"):
            means(*args)
    with pytest.raises(ValueError, match="8-byte aligned"):
        means(a + 4, None, 4, a, None, a, a, a, a, a, a, a, 64, 0)
    with pytest.raises(ValueError, match="flat rows must be 4-byte aligned"):
        means(a, None, 4, a, None, a, a, a + 2, a, a, a, a, 64, 0)
    with pytest.raises(ValueError, match="2\\^38"):
        means(a, None, 4, a, None, a, a, a, a, a, a, a, 1 << 38, 0)
    means(None, None, 4, None, None, None, None, None, None, None, None, None, 0, 0)  # D = 0: no launch

    # rows_dots: (rows, R, vecs, m, D, workspace, out, stream)
    dots = lambda *args: _lib.call("plato_agg_rows_dots", *args, None)  # noqa: E731
    for r in (0, 65537, -1):
        with pytest.raises(ValueError, match=r"R must be in 1\.\.65536"):
            dots(a, r, a, 3, 64, a, a)
    for m in (0, 5, -1):
        with pytest.raises(ValueError, match=r"m must be in 1\.\.4"):
            dots(a, 4, a, m, 64, a, a)
    for args in ((None, 4, a, 3, 64, a, a), (a, 4, None, 3, 64, a, a)):
        with pytest.raises(ValueError, match="null pointer table"):
            dots(*args)
    for args in ((a, 4, a, 3, 64, None, a), (a, 4, a, 3, 64, a, None)):
        with pytest.raises(ValueError, match="null output or workspace"):
            dots(*args)
    with pytest.raises(ValueError, match="8-byte aligned"):
        dots(a + 4, 4, a, 3, 64, a, a)
    with pytest.raises(ValueError, match="16-byte aligned"):
        dots(a, 4, a, 3, 64, a, a + 8)
    with pytest.raises(ValueError, match="256-byte aligned"):
        dots(a, 4, a, 3, 64, a + 128, a)
    with pytest.raises(ValueError, match="2\\^38"):
        dots(a, 4, a, 3, 1 << 38, a, a)
    dots(None, 4, None, 3, 0, a, a)  # D = 0: no launch

    # lbfgs_predict: (rows, R, a, sigma, last_g, v, pred, D, stream)
    pred = lambda *args: _lib.call("plato_agg_lbfgs_predict", *args, None)  # noqa: E731
    with pytest.raises(ValueError, match=r"R must be in 1\.\.65536"):
        pred(a, 0, a, 1.0, a, a, a, 64)
    for args in ((None, 2, a, 1.0, a, a, a, 64), (a, 2, None, 1.0, a, a, a, 64)):
        with pytest.raises(ValueError, match="null pointer table"):
            pred(*args)
    for hole in (4, 5, 6):
        args = [a, 2, a, 1.0, a, a, a, 64]
        args[hole] = None
        with pytest.raises(ValueError, match="null flat row"):
            pred(*args)
    with pytest.raises(ValueError, match="8-byte aligned"):
        pred(a, 2, a + 4, 1.0, a, a, a, 64)
    with pytest.raises(ValueError, match="4-byte aligned"):
        pred(a, 2, a, 1.0, a, a, a + 1, 64)
    pred(None, 2, None, 1.0, None, None, None, 0)  # D = 0: no launch

    # delta_sqdist: (x_f32, x_i64, K, b_f32, b_i64, pred, n_f32, n_i64, workspace, out, stream)
    dist = lambda *args: _lib.call("plato_agg_delta_sqdist", *args, None)  # noqa: E731
    for k in (0, 257):
        with pytest.raises(ValueError, match=r"K must be in 1\.\.256"):
            dist(a, None, k, a, None, a, 64, 0, a, a)
    with pytest.raises(ValueError, match="null fp32"):
        dist(None, None, 4, a, None, a, 64, 0, a, a)
    with pytest.raises(ValueError, match="null int64"):
        dist(a, a, 4, a, None, a, 64, 1, a, a)
    with pytest.raises(ValueError, match="null flat row"):
        dist(a, None, 4, a, None, None, 64, 0, a, a)
    with pytest.raises(ValueError, match="null output or workspace"):
        dist(a, None, 4, a, None, a, 64, 0, None, a)
    with pytest.raises(ValueError, match="baseline must be"):
        dist(a, a, 4, a, a + 4, a, 64, 1, a, a)
    with pytest.raises(ValueError, match="16-byte aligned"):
        dist(a, None, 4, a, None, a, 64, 0, a, a + 8)
    dist(None, None, 4, None, None, None, 0, 0, a, a)  # D = 0: no launch
