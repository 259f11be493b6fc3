"""FLDetector on the GPU: the four kernels of plato_amd/csrc/detect.hip against the numpy restatement
(tests/fldetector_oracle.py), and the engine and the server hook against the reference fixtures
(tests/golden/fldetector_*).

Shape of the reductions that the sizes below walk around: workgroups of 256 lanes take 512 coordinates per
pass and 8 rows per batch; a chunk is PLATO_AGG_TRUST_TILE = 1,024 coordinates for models this small, one
workgroup per (chunk, batch).  rows_dots chunks the flat row as a whole, delta_sqdist the fp32 region and
the int64 region apart.

The means and the prediction are compared bit for bit.  The dots and the squared distances are compared
with ``math.fsum`` of the same float64 terms within property (c) of the header, D * 2^-53 * sum|terms|
(derived from the summation, not measured), and must be bitwise repeatable, bitwise permuted under a
permuted pointer table and unchanged for one row when the others change.
"""

import asyncio
import types

import numpy as np
import pytest
import torch

from plato_amd import _lib
from plato_amd import detectors as host
from plato_amd.engine import AggregationRound, FedAvgEngine
from plato_amd.servers import AttackSimulationMixin, DetectorFilterMixin, TrustAggregationMixin, make_server
from tests import fldetector_cases as fc
from tests import fldetector_oracle as fo
from tests.test_fldetector import NAMES, ROUNDS, bits, case_of, full_arrays, layout_index

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TILE = _lib.PLATO_AGG_TRUST_TILE
SENTINEL = -7.0
NS = (1, 63, 64, 65, 511, 512, 513, 1023, 1025, 2049, 3 * TILE + 77)  # the last: four chunks, a ragged one
NIS = (0, 1, 3)
KS = (1, 3, 8, 9, 17)
RECORDS = (1, 2, 3, 9)
MS = (1, 3, 4)
# every size once, the other parameters cycling beside it; then every K and N at the several-chunk size
SHAPES = [(n, NIS[i % 3], KS[i % 5], RECORDS[i % 4]) for i, n in enumerate(NS)]
SHAPES += [(NS[-1], NIS[(i + 1) % 3], k, RECORDS[(i + 2) % 4]) for i, k in enumerate(KS)]
SHAPES += [(1025, 3, 9, 9), (513, 1, 17, 1)]


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def table(ptrs):
    return torch.tensor(list(ptrs), dtype=torch.int64, device=DEV)


def client_tables(xf, xi, order=None):
    k, n_f, n_i = xf.shape[0], xf.shape[1], xi.shape[1]
    order = range(k) if order is None else order
    df, di = dev(xf), dev(xi)
    return (df, di), table(df.data_ptr() + 4 * n_f * c for c in order), table(di.data_ptr() + 8 * n_i * c for c in order)


def guarded(n, dtype=torch.float32):
    """n elements to be written, 64 guard elements behind them."""
    return torch.full((n + 64,), SENTINEL, dtype=dtype, device=DEV)


def unguard(t, n):
    assert bool((t[n:] == SENTINEL).all()), "the kernel wrote past its output"
    return t[:n].cpu().numpy()


def inputs(rng, k, n_f, n_i):
    bf = rng.standard_normal(n_f).astype(np.float32)
    bi = rng.integers(0, 10001, n_i, dtype=np.int64)
    xf = (bf + np.float32(0.25) * rng.standard_normal((k, n_f)).astype(np.float32)).astype(np.float32)
    xi = bi + rng.integers(-3, 9, (k, n_i), dtype=np.int64)
    d = n_f + n_i
    last_w = (0.5 * rng.standard_normal(d)).astype(np.float32)
    last_g = (0.1 * rng.standard_normal(d)).astype(np.float32)
    return bf, bi, xf, xi, last_w, last_g


def device_means(bf, bi, xf, xi, last_w, last_g):
    k, n_f, n_i = xf.shape[0], xf.shape[1], xi.shape[1]
    d = n_f + n_i
    keep, tf, ti = client_tables(xf, xi)
    dbf, dbi, dw, dg = dev(bf), dev(bi), dev(last_w), dev(last_g)
    outs = [guarded(d) for _ in range(5)]
    _lib.call("plato_agg_detect_means", tf.data_ptr() if n_f else None, ti.data_ptr() if n_i else None, k,
              dbf.data_ptr() if n_f else None, dbi.data_ptr() if n_i else None, dw.data_ptr(), dg.data_ptr(),
              *(o.data_ptr() for o in outs), n_f, n_i, stream())
    torch.cuda.synchronize()
    del keep
    return [unguard(o, d) for o in outs]


def device_dots(rows, vecs, order=None):
    """plato_agg_rows_dots of host rows [R, D] and vectors [m, D]; sentinel guards behind output and workspace."""
    r, d, m = rows.shape[0], rows.shape[1], vecs.shape[0]
    order = range(r) if order is None else order
    dr, dv = dev(rows), dev(vecs)
    rt, vt = table(dr.data_ptr() + 4 * d * j for j in order), table(dv.data_ptr() + 4 * d * j for j in range(m))
    nbytes = _lib.lib().plato_agg_rows_dots_workspace(r, m, d)
    assert nbytes >= r * m * 8
    words = (nbytes + 7) // 8
    work, out = guarded(words, torch.float64), guarded(r * m, torch.float64)
    _lib.call("plato_agg_rows_dots", rt.data_ptr(), r, vt.data_ptr(), m, d, work.data_ptr(), out.data_ptr(), stream())
    torch.cuda.synchronize()
    unguard(work, words)
    return unguard(out, r * m).reshape(r, m)


def device_predict(rows, a, sigma, last_g, v):
    r, d = rows.shape
    dr, da, dg, dv = dev(rows), dev(np.asarray(a, dtype=np.float64)), dev(last_g), dev(v)
    rt = table(dr.data_ptr() + 4 * d * j for j in range(r))
    pred = guarded(d)
    _lib.call("plato_agg_lbfgs_predict", rt.data_ptr(), r, da.data_ptr(), float(sigma), dg.data_ptr(), dv.data_ptr(),
              pred.data_ptr(), d, stream())
    torch.cuda.synchronize()
    return unguard(pred, d)


def device_sqdist(bf, bi, xf, xi, pred, order=None):
    k, n_f, n_i = xf.shape[0], xf.shape[1], xi.shape[1]
    keep, tf, ti = client_tables(xf, xi, order)
    dbf, dbi, dp = dev(bf), dev(bi), dev(pred)
    nbytes = _lib.lib().plato_agg_delta_sqdist_workspace(k, n_f, n_i)
    words = (nbytes + 7) // 8
    work, out = guarded(words, torch.float64), guarded(k, torch.float64)
    _lib.call("plato_agg_delta_sqdist", tf.data_ptr() if n_f else None, ti.data_ptr() if n_i else None, k,
              dbf.data_ptr() if n_f else None, dbi.data_ptr() if n_i else None, dp.data_ptr(), n_f, n_i,
              work.data_ptr(), out.data_ptr(), stream())
    torch.cuda.synchronize()
    unguard(work, words)
    del keep
    return unguard(out, k)


def within(got, exp, mag, d):
    err = np.abs(got - exp)
    assert np.all(err <= fo.bound(d, mag)), float(np.max(err / np.maximum(fo.bound(d, mag), 1e-300)))


# ------------------------------------------------------------------ the kernels at the seams
@pytest.mark.parametrize("n_f,n_i,k,n", SHAPES)
def test_means_prediction_and_distances_at_the_seams(n_f, n_i, k, n):
    rng = np.random.default_rng(1000 * n_f + 100 * n_i + 10 * k + n)
    bf, bi, xf, xi, last_w, last_g = inputs(rng, k, n_f, n_i)
    d = n_f + n_i
    exp = fo.detect_means(xf, xi, bf, bi, last_w, last_g)
    got = device_means(bf, bi, xf, xi, last_w, last_g)
    for name, g, e in zip(("g", "v", "s_new", "y_new", "b_flat"), got, exp):
        assert np.array_equal(bits(g), bits(e)), name
    # the prediction over 2N record rows
    rows = (0.3 * rng.standard_normal((2 * n, d))).astype(np.float32)
    a, sigma = rng.standard_normal(2 * n), float(rng.uniform(0.5, 2.0))
    pred = device_predict(rows, a, sigma, last_g, exp[1])
    assert np.array_equal(bits(pred), bits(fo.predict(list(rows), a, sigma, last_g, exp[1])))
    # the distances of the deltas to it
    d2, mag = fo.sqdist(pred, fo.deltas(xf, xi, bf, bi))
    got = device_sqdist(bf, bi, xf, xi, pred)
    within(got, d2, mag, d)
    assert np.array_equal(bits(got), bits(device_sqdist(bf, bi, xf, xi, pred)))  # repeatable
    order = list(rng.permutation(k))
    assert np.array_equal(bits(device_sqdist(bf, bi, xf, xi, pred, order)), bits(got[order]))
    if k > 1:  # client 0's value does not depend on the other rows, nor on K
        other_f, other_i = xf.copy(), xi.copy()
        other_f[1:] = -other_f[1:] + 1
        other_i[1:] += 5
        assert bits(device_sqdist(bf, bi, other_f, other_i, pred)[0]) == bits(got[0])
        assert bits(device_sqdist(bf, bi, xf[:1], xi[:1], pred)[0]) == bits(got[0])


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("d,r", [(n, 2 * RECORDS[i % 4] + 2) for i, n in enumerate(NS)] + [(NS[-1], 17), (1025, 8)])
def test_rows_dots_at_the_seams(d, r, m):
    rng = np.random.default_rng(77 * d + 7 * r + m)
    rows = rng.standard_normal((r, d)).astype(np.float32)
    vecs = rng.standard_normal((m, d)).astype(np.float32)
    exp, mag = fo.rows_dots(list(rows), list(vecs))
    got = device_dots(rows, vecs)
    within(got, exp, mag, d)
    assert np.array_equal(bits(got), bits(device_dots(rows, vecs)))  # repeatable
    order = list(rng.permutation(r))
    assert np.array_equal(bits(device_dots(rows, vecs, order)), bits(got[order]))
    # (row, vector) depends on that row, that vector and D alone: not on the other rows, on R or on m
    other = rows.copy()
    other[1:] = 2 * other[1:] + 1
    assert np.array_equal(bits(device_dots(other, vecs)[0]), bits(got[0]))
    assert np.array_equal(bits(device_dots(rows[:1], vecs[:1])[0, 0]), bits(got[0, 0]))
    # and the two may change places (the Gram cache takes S Y^T from either side)
    assert np.array_equal(bits(device_dots(vecs, rows[:1])[:, 0]), bits(got[0]))


def test_a_nan_and_an_infinity_reach_only_their_clients_distance():
    rng = np.random.default_rng(3)
    n_f, n_i, k = TILE + 5, 3, 9
    bf, bi, xf, xi, _, last_g = inputs(rng, k, n_f, n_i)
    xf[2, TILE + 1] = np.nan
    xf[7, 3] = np.inf
    pred = (0.1 * rng.standard_normal(n_f + n_i)).astype(np.float32)
    got = device_sqdist(bf, bi, xf, xi, pred)
    assert np.isnan(got[2]) and got[7] == np.inf
    rest = [c for c in range(k) if c not in (2, 7)]
    exp, mag = fo.sqdist(pred, fo.deltas(xf, xi, bf, bi))
    assert np.all(np.isfinite(got[rest]))
    within(got[rest], exp[rest], mag[rest], n_f + n_i)
    # and in the dots: a row's NaN stays in that row, a vector's reaches every row
    rows = rng.standard_normal((5, 700)).astype(np.float32)
    vecs = rng.standard_normal((3, 700)).astype(np.float32)
    rows[1, 699], rows[3, 0] = np.nan, -np.inf
    got = device_dots(rows, vecs)
    assert np.all(np.isnan(got[1])) and np.all(np.isinf(got[3])) and np.all(np.isfinite(got[[0, 2, 4]]))
    vecs[2, 5] = np.nan
    got = device_dots(rows, vecs)
    assert np.all(np.isnan(got[:, 2])) and np.all(np.isfinite(got[[0, 2, 4]][:, :2]))


def test_values_near_1e30_neither_overflow_nor_flush_in_float64():
    rng = np.random.default_rng(4)
    d = 1025
    big = (rng.standard_normal((3, d)) * 1e30).astype(np.float32)
    tiny = (rng.standard_normal((3, d)) * 1e-30).astype(np.float32)
    for rows, vecs in ((big, big), (tiny, tiny), (big, tiny)):
        exp, mag = fo.rows_dots(list(rows), list(vecs))
        got = device_dots(rows, vecs)
        assert np.all(np.isfinite(got)) and np.all(got != 0)
        within(got, exp, mag, d)
    assert device_dots(big, big)[0, 0] > 1e62 and 0 < device_dots(tiny, tiny)[0, 0] < 1e-56
    # squared distances of deltas near 1e30 to a prediction near -1e30; and of tiny ones
    for scale in (1e30, 1e-30):
        bf = np.zeros(d, dtype=np.float32)
        xf = (rng.standard_normal((3, d)) * scale).astype(np.float32)
        pred = (-rng.standard_normal(d) * scale).astype(np.float32)
        xi = np.zeros((3, 0), dtype=np.int64)
        exp, mag = fo.sqdist(pred, fo.deltas(xf, xi, bf, np.zeros(0, dtype=np.int64)))
        got = device_sqdist(bf, np.zeros(0, dtype=np.int64), xf, xi, pred)
        assert np.all(np.isfinite(got)) and np.all(got > 0)
        within(got, exp, mag, d)


# ------------------------------------------------------------------ the engine against the reference
@pytest.fixture(scope="module")
def engine():
    return FedAvgEngine(DEV)


def staged_round(engine, lay, bf, bi, xf, xi):
    baseline = fc.state_dict(lay, bf, bi)
    rnd = engine.begin(baseline, xf.shape[0])
    rnd.deltas = False
    rnd.put_baseline(baseline)
    for slot in range(xf.shape[0]):
        rnd.put_client(slot, fc.state_dict(lay, xf[slot], xi[slot]))
    return rnd


@pytest.mark.parametrize("name,t", ROUNDS)
def test_a_round_from_the_references_record_is_within_its_own_error(engine, name, t):
    case = case_of(name)
    lay, _ = layout_index(name)
    state = host.FLDetectorState()
    state.load_reference_record(*fc.reference_record(case, full_arrays(), t, lay), lay)
    engine.fldetector = state
    bf, bi, xf, xi, ids = fc.scenario(name)[t]
    rnd = staged_round(engine, lay, bf, bi, xf, xi)
    rnd.launch_fldetector(ids)
    got, expected = rnd.detector, case["rounds"][t]
    exact = fc.f64s(expected["exact"])
    err = float(np.max(np.abs(np.sqrt(got["d2"]) - exact) / exact))
    print(f"{name} round {t}: err {err:.3e}, ref_err {expected['ref_err']:.3e}, cond {got['cond']:.3e}")
    assert err <= expected["ref_err"]
    assert got["malicious"] == sorted(expected["malicious"])
    assert got["records"] == t and len(state) == t + 1
    for key in ("detect_means_ms", "rows_dots_ms", "lbfgs_predict_ms", "delta_sqdist_ms", "detector_gram_ms"):
        assert rnd.timings[key] >= 0
    n_f = lay.n_f32
    assert got["pred"][0].shape == (n_f,) and got["pred"][1].shape == (lay.n_i64,)
    engine.fldetector = None


def test_a_singular_record_raises_and_leaves_the_state_as_it_was(engine):
    name = "fld_bn_k8_a2"
    lay, _ = layout_index(name)
    bf, bi, xf, xi, ids = fc.scenario(name)[0]
    engine.fldetector = None
    for _ in range(2):  # two identical rounds: y_last = 0
        staged_round(engine, lay, bf, bi, xf, xi).launch_fldetector(ids)
    state = engine.fldetector
    assert len(state) == 2 and state.yy[1] == 0.0
    before = (state.sy.copy(), [r.data_ptr() for r in state.s_rows], state.last_g.data_ptr(), dict(state.history))
    with pytest.raises(ValueError, match="not finite"):
        staged_round(engine, lay, bf, bi, xf, xi).launch_fldetector(ids)
    assert len(state) == 2 and np.array_equal(state.sy, before[0]) and state.last_g.data_ptr() == before[2]
    assert [r.data_ptr() for r in state.s_rows] == before[1] and state.history == before[3]
    with pytest.raises(ValueError, match="client ids"):
        staged_round(engine, lay, bf, bi, xf, xi).launch_fldetector(ids[:-1])
    rnd = engine.begin(fc.state_dict(lay, bf, bi), 1)
    rnd.deltas = False
    rnd.put_client(0, fc.state_dict(lay, xf[0], xi[0]))
    with pytest.raises(ValueError, match="stage the baseline first"):
        rnd.launch_fldetector(ids[:1])
    engine.fldetector = None


# ------------------------------------------------------------------ whole scenarios through the server hook
class _Base:
    """What the hooks need of the detector server."""

    def weights_attacked(self, weights_received):
        return weights_received

    def weights_filter(self, weights_attacked):
        raise AssertionError("FLDetector is the mixin's")


class _Mixin(DetectorFilterMixin, AttackSimulationMixin, TrustAggregationMixin):
    pass


def flat_result(lay, result):
    return np.concatenate([result[e.name].reshape(-1).numpy() for reg in ("f32", "i64")
                           for e in lay.entries if e.region == reg])


@pytest.mark.parametrize("name", NAMES)
def test_a_whole_scenario_through_the_server_hook(name, monkeypatch):
    case = case_of(name)
    lay, index = layout_index(name)
    server = make_server(base=_Base, mixin=_Mixin)()
    server.aggregation_device = "cuda:0"
    server.secure_aggregation_type = "Fl-trust"
    server.detector_type = "FLDetector"
    server.attack_simulation_type = "Fang"  # the base class's: the scenario's payloads are poisoned already
    server.attacker_list = list(case["recipe"]["attackers"])
    plain = FedAvgEngine(DEV)
    puts = []
    put_client = AggregationRound.put_client
    monkeypatch.setattr(AggregationRound, "put_client", lambda self, *a, **kw: (puts.append(self), put_client(self, *a, **kw))[1])
    worst = 0.0
    for t, (bf, bi, xf, xi, ids) in enumerate(fc.scenario(name)):
        expected = case["rounds"][t]
        server.updates = [types.SimpleNamespace(client_id=i, report=types.SimpleNamespace(num_samples=10)) for i in ids]
        server.algorithm = types.SimpleNamespace(extract_weights=lambda bf=bf, bi=bi: fc.state_dict(lay, bf, bi))
        payloads = [fc.state_dict(lay, xf[c], xi[c]) for c in range(len(ids))]
        approved = server.weights_filter(server.weights_attacked(payloads))
        flagged = sorted(expected["malicious"])
        assert server._plato_amd_detector["malicious"] == flagged, t
        keep = [c for c in range(len(ids)) if c not in flagged]
        assert len(approved) == len(keep) and all(approved[j] is payloads[c] for j, c in enumerate(keep))
        if t:
            ref, got = fc.hexes(expected["normalised"]), server._plato_amd_detector["distances"]
            worst = max(worst, float(np.max(np.abs(got.astype(np.float64) - ref.astype(np.float64)))))
        # the aggregation that follows adopts the rows the filter staged: it stages nothing itself
        engine = server.aggregation_engine()
        assert all(engine._arrivals.lookup(p, "native", lay.signature) is not None for p in payloads)
        staged_before = len(puts)
        result = asyncio.run(server.aggregate_weights(server.updates, None, approved))
        assert len(puts) == staged_before and len(engine._arrivals) == 0
        alone = plain.aggregate_fltrust(approved)
        assert np.array_equal(bits(flat_result(lay, result)), bits(flat_result(lay, alone))), t
    print(f"{name}: max |normalised distance - reference's| over the scenario {worst:.3e}")
    state = server.aggregation_engine().fldetector
    assert len(state) == case["recipe"]["rounds"] and state.rounds == len(state)
    sy, ss, yy = state.full_gram(torch.cuda.current_stream(DEV))
    assert np.array_equal(bits(sy), bits(state.sy)) and np.array_equal(bits(ss), bits(state.ss))
    assert np.array_equal(bits(yy), bits(state.yy))
    # the checkpoint of a device-resident record restores the same rows and cache
    again = host.FLDetectorState()
    again.load_state_dict(state.state_dict())
    assert np.array_equal(bits(again.sy), bits(state.sy)) and len(again) == len(state)
    assert all(np.array_equal(bits(a.numpy()), bits(b.cpu().numpy())) for a, b in zip(again.y_rows, state.y_rows))


def test_the_filter_adopts_the_rows_a_device_side_attack_poisoned(monkeypatch):
    """Lambda attack on the device, then the filter, then Fl-trust: the filter stages only the clients the
    attack did not, and the aggregate is that of the approved (written-back) payloads alone."""
    name = "fld_bn_k8_a2"
    lay, _ = layout_index(name)
    server = make_server(base=_Base, mixin=_Mixin)()
    server.aggregation_device = "cuda:0"
    server.secure_aggregation_type = "Fl-trust"
    server.detector_type = "FLDetector"
    server.attack_simulation_type = "Lambda_attack"
    server.attack_lambada_value = 2
    server.attacker_list = [2, 7]
    plain = FedAvgEngine(DEV)
    engine = server.aggregation_engine()
    prestaged = []
    prestage = engine.prestage
    monkeypatch.setattr(engine, "prestage", lambda p, *a, **kw: (prestaged.append(p), prestage(p, *a, **kw))[1])
    puts = []
    put_client = AggregationRound.put_client
    monkeypatch.setattr(AggregationRound, "put_client", lambda self, *a, **kw: (puts.append(self), put_client(self, *a, **kw))[1])
    for t, (bf, bi, xf, xi, ids) in enumerate(fc.scenario(name)[:3]):
        server.updates = [types.SimpleNamespace(client_id=i, report=types.SimpleNamespace(num_samples=10)) for i in ids]
        server.algorithm = types.SimpleNamespace(extract_weights=lambda bf=bf, bi=bi: fc.state_dict(lay, bf, bi))
        payloads = [fc.state_dict(lay, xf[c], xi[c]) for c in range(len(ids))]
        attackers = [payloads[c] for c, i in enumerate(ids) if i in server.attacker_list]
        clean = [[v.clone() for v in p.values()] for p in attackers]
        attacked = server.weights_attacked(payloads)
        assert server._plato_amd_attack["poisoned"] and len(prestaged) == 2
        assert all(any(not torch.equal(a, b) for a, b in zip(p.values(), c)) for p, c in zip(attackers, clean))
        approved = server.weights_filter(attacked)
        # the filter adopted the attackers' poisoned rows and staged the other six as arrival rows
        assert len(prestaged) == len(ids) and all(p is not q for p in prestaged[2:] for q in attackers)
        flagged = server._plato_amd_detector["malicious"]
        assert [id(p) for p in approved] == [id(p) for c, p in enumerate(payloads) if c not in flagged]
        result = asyncio.run(server.aggregate_weights(server.updates, None, approved))
        assert not puts and len(engine._arrivals) == 0
        alone = plain.aggregate_fltrust(approved)
        assert np.array_equal(bits(flat_result(lay, result)), bits(flat_result(lay, alone))), t
        prestaged.clear()
        puts.clear()


def test_a_window_keeps_the_newest_records(engine):
    name = "fld_mlp_k9_a0"
    lay, _ = layout_index(name)
    engine.fldetector = host.FLDetectorState(max_records=2)
    for bf, bi, xf, xi, ids in fc.scenario(name)[:5]:
        staged_round(engine, lay, bf, bi, xf, xi).launch_fldetector(ids)
    state = engine.fldetector
    assert len(state) == 2 and state.rounds == 5 and state.sy.shape == (2, 2)
    sy, ss, yy = state.full_gram(torch.cuda.current_stream(DEV))
    assert np.array_equal(bits(sy), bits(state.sy)) and np.array_equal(bits(ss), bits(state.ss))
    assert np.array_equal(bits(yy), bits(state.yy))
    engine.fldetector = None
