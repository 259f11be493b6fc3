"""The attack simulation on the GPU: plato_agg_column_std and plato_agg_add_scaled_rows against the numpy
restatements (tests/attack_oracle.py), and the engine and the server hook against the reference fixtures
(tests/golden/attack_*).

Shape of the kernels (plato_amd/csrc/attack.hip) that the sizes below walk around: workgroups of 256 lanes,
four consecutive coordinates per lane (a tile of 1,024), read as one 16-byte load where the row is 16-byte
aligned and as four 4-byte loads where it is not; rows taken four at a time.  The rows of a test matrix lie
back to back, so with a coordinate count that is no multiple of four every second or fourth row is
misaligned and both loads run in one launch.  The counters go one (add_scaled_rows) or four (column_std)
per lane.
"""

import types

import numpy as np
import pytest
import torch

from plato_amd import _lib
from plato_amd.engine import FedAvgEngine
from plato_amd.servers import AttackSimulationMixin, DetectorAggregationMixin, make_server
from tests import attack_cases as ac
from tests import attack_oracle as ao
from tests import krum_oracle as ko
from tests.attack_cases import bits, case_of, inputs

CASES, NAMES = ac.cases(), ac.names()

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TILE = 1024
MS = (1, 2, 3, 20, 33, 255, 256)
NS = (1, 3, 4, 255, 1025, TILE - 1, TILE, 2 * TILE + 3, 0)
NIS = (0, 1, 5)
SENTINEL = -7.0


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def tables(xf: np.ndarray, xi: np.ndarray, order=None):
    k, n_f, n_i = xf.shape[0], xf.shape[1], xi.shape[1]
    order = range(k) if order is None else order
    df = torch.from_numpy(np.ascontiguousarray(xf)).to(DEV)
    di = torch.from_numpy(np.ascontiguousarray(xi)).to(DEV)
    tf = torch.tensor([df.data_ptr() + 4 * n_f * c for c in order], dtype=torch.int64, device=DEV)
    ti = torch.tensor([di.data_ptr() + 8 * n_i * c for c in order], dtype=torch.int64, device=DEV)
    return (df, di), tf, ti


def device_std(xf, xi, order=None):
    """plato_agg_column_std of [m, n] host matrices; 64 sentinel elements follow each output."""
    n_f, n_i = xf.shape[1], xi.shape[1]
    keep, tf, ti = tables(xf, xi, order)
    out_f = torch.full((n_f + 64,), SENTINEL, device=DEV)
    out_i = torch.full((n_i + 64,), SENTINEL, device=DEV)
    _lib.call("plato_agg_column_std", tf.data_ptr() if n_f else None, ti.data_ptr() if n_i else None, tf.numel(),
              out_f.data_ptr() if n_f else None, out_i.data_ptr() if n_i else None, n_f, n_i, stream())
    torch.cuda.synchronize()
    assert bool((out_f[n_f:] == SENTINEL).all()) and bool((out_i[n_i:] == SENTINEL).all())
    del keep
    return np.concatenate([out_f[:n_f].cpu().numpy(), out_i[:n_i].cpu().numpy()])


def device_add(xf, xi, s, v, order=None):
    """plato_agg_add_scaled_rows on [m, n] host matrices: the matrices afterwards, every row included."""
    n_f, n_i = xf.shape[1], xi.shape[1]
    (df, di), tf, ti = tables(xf, xi, order)
    vf = torch.from_numpy(np.ascontiguousarray(v[:n_f])).to(DEV)
    vi = torch.from_numpy(np.ascontiguousarray(v[n_f:])).to(DEV)
    _lib.call("plato_agg_add_scaled_rows", tf.data_ptr() if n_f else None, ti.data_ptr() if n_i else None, tf.numel(),
              float(s), vf.data_ptr() if n_f else None, vi.data_ptr() if n_i else None, n_f, n_i, stream())
    torch.cuda.synchronize()
    return df.cpu().numpy(), di.cpu().numpy()


def rows(rng, m: int, n_f: int, n_i: int):
    base = rng.standard_normal(n_f).astype(np.float32)
    xf = (base + np.float32(0.25) * rng.standard_normal((m, n_f)).astype(np.float32)).astype(np.float32)
    xi = rng.integers(0, 10001, n_i, dtype=np.int64) + rng.integers(-9, 9, (m, n_i), dtype=np.int64)
    return xf, xi


def sizes():
    for n_f in NS:
        for n_i in NIS:
            if n_f or n_i:
                yield n_f, n_i


def same(got, exp):
    """Bit for bit, a NaN for a NaN (the sign and payload of a NaN are the platform's)."""
    got, exp = np.asarray(got, dtype=np.float32), np.asarray(exp, dtype=np.float32)
    nan = np.isnan(exp)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got[~nan]), bits(exp[~nan]))


# ------------------------------------------------------------------ plato_agg_column_std
@pytest.mark.parametrize("m", MS)
def test_column_std_equals_the_welford_restatement_bit_for_bit(m):
    rng = np.random.default_rng(9000 + m)
    for n_f, n_i in sizes():
        xf, xi = rows(rng, m, n_f, n_i)
        got = device_std(xf, xi)
        exp = ao.column_std(ao.columns(xf, xi))
        assert same(got, exp), (m, n_f, n_i)
        if m == 1:
            assert np.isnan(got).all()


def test_column_std_follows_the_table_order_and_ignores_other_rows():
    rng = np.random.default_rng(9100)
    xf, xi = rows(rng, 33, 1025, 5)
    perm = list(rng.permutation(33)[:20])
    got = device_std(xf, xi, order=perm)
    assert same(got, ao.column_std(ao.columns(xf[perm], xi[perm])))


def test_column_std_special_values():
    rng = np.random.default_rng(9200)
    m, n_f, n_i = 5, TILE + 1, 5
    xf, xi = rows(rng, m, n_f, n_i)
    clean = device_std(xf, xi)
    xf[:, 7] = np.float32(1.25)           # identical rows: exactly +0
    xf[:, 8] = np.float32(-0.0)
    xf[2, TILE] = np.nan                  # the last coordinate, in the second tile
    xf[1, 17] = np.inf
    xf[3, 18] = -np.inf
    xf[:, 19] = np.float32(3.4e38) * np.float32([1, -1, 1, -1, 1])  # the deviation overflows at the cast only
    xf[:, 20] = np.float32(3.4e38)        # near FLT_MAX and equal: +0, nothing overflows on the way
    xf[:, 21] = np.float32([1e-45, 3e-45, 0, 7e-45, 1e-44])      # subnormals
    xf[:, 22] = np.float32([1e-38, 1e-38, 1.00001e-38, 1e-38, 1e-38])
    xi[:, 0] = (1 << 24) + np.arange(m)   # counters above 2^24: promoted with round to nearest even
    xi[:, 1] = [(1 << 25) + 1, (1 << 25) + 3, -(1 << 25) - 1, 5, (1 << 40) + 1]
    got = device_std(xf, xi)
    exp = ao.column_std(ao.columns(xf, xi))
    assert same(got, exp)
    assert not bits(got[[7, 8, 20]]).any()
    assert np.isnan(got[[TILE, 17, 18]]).all() and got[19] == np.inf
    assert 0 < got[21] < 1e-44 and 0 < got[22] < 1e-42
    assert got[n_f] == ao.column_std(xi[:, :1].astype(np.float32))[0] and got[n_f] != np.float32(np.std(np.arange(m), ddof=1))
    touched = np.array([7, 8, TILE, 17, 18, 19, 20, 21, 22, n_f, n_f + 1])
    others = np.setdiff1d(np.arange(n_f + n_i), touched)
    assert np.array_equal(bits(got[others]), bits(clean[others]))  # a NaN stays in its own coordinate


# ------------------------------------------------------------------ plato_agg_add_scaled_rows
@pytest.mark.parametrize("m", (1, 2, 20))
def test_add_scaled_rows_equals_the_restatement_bit_for_bit(m):
    rng = np.random.default_rng(9300 + m)
    for n_f, n_i in sizes():
        xf, xi = rows(rng, m + 2, n_f, n_i)
        v = np.concatenate([rng.standard_normal(n_f), rng.standard_normal(n_i) * 7]).astype(np.float32)
        s = np.float32(-0.7549029)
        order = list(range(1, m + 1))     # rows 0 and m + 1 are not in the table
        got_f, got_i = device_add(xf, xi, s, v, order)
        exp_f, exp_i = ao.add_scaled_rows(xf[order], xi[order], s, v)
        assert np.array_equal(bits(got_f[order]), bits(exp_f)) and np.array_equal(got_i[order], exp_i), (m, n_f, n_i)
        for r in (0, m + 1):
            assert np.array_equal(bits(got_f[r]), bits(xf[r])) and np.array_equal(got_i[r], xi[r])


def test_add_scaled_rows_counters_truncate_toward_zero_and_saturate():
    v = np.float32([0.5, 2.75, -2.75, 0.99, -0.99, np.nan, 1e30, -1e30, 9.3e18, -9.3e18, 2.0 ** 62, 3.0])
    n_f, n_i = 1, v.size - 1
    xf = np.float32([[1.0], [2.0], [-0.0]])
    xi = np.tile(np.array([[10], [-7], [(1 << 62) + 5]], dtype=np.int64), (1, n_i))
    for s in (np.float32(1.0), np.float32(-1.0), np.float32(-1.5)):
        got_f, got_i = device_add(xf, xi, s, v)
        exp_f, exp_i = ao.add_scaled_rows(xf, xi, s, v)
        assert np.array_equal(bits(got_f), bits(exp_f)) and np.array_equal(got_i, exp_i)
    got_f, got_i = device_add(xf, xi, np.float32(-1.0), v)
    low = np.iinfo(np.int64).min
    assert got_i[0].tolist()[:4] == [8, 12, 10, 10]          # -2.75 -> -2, 2.75 -> 2, -+0.99 -> 0
    assert got_i[0, 4] == low + 10 and got_i[0, 5] == low + 10 and got_i[0, 6] == low + 10  # NaN, -+1e30
    assert got_i[0, 7] == low + 10 and got_i[0, 8] == low + 10                               # -+9.3e18 > 2^63
    assert got_i[2, 9] == 5 and got_i[0, 10] == 7            # -2^62 exactly; -3
    assert bits(got_f[2])[0] == bits(np.float32([-0.5]))[0]


def test_add_scaled_rows_special_values_in_the_fp32_region():
    xf = np.float32([[0.0, -0.0, np.inf, 1e-45, 3e38, 1.0], [-0.0, 0.0, -np.inf, -1e-45, -3e38, np.nan]])
    xi = np.zeros((2, 0), dtype=np.int64)
    for s, v in ((np.float32(0.0), np.float32([1, -1, 1, 1, 1, 1])), (np.float32(2.0), np.float32([0, -0.0, -np.inf, 1e-45, 3e38, 1])),
                 (np.float32(np.inf), np.float32([0, 1, 1, 1, 1, 1]))):
        got_f, _ = device_add(xf, xi, s, v)
        assert same(got_f, ao.add_scaled_rows(xf, xi, s, v)[0])


# ------------------------------------------------------------------ engine, end to end on the fixtures
@pytest.fixture(scope="module")
def engine():
    return FedAvgEngine(DEV)


def run_attack(engine, name, extra=0):
    """The attack of a case on the engine: (poisoned fp32 [A, n], poisoned int64, the round's scalars and
    its vector on the host).  ``extra`` clients that are no attackers are staged behind them."""
    r = case_of(name)["recipe"]
    layout, bf, bi, wf, wi, _ = inputs(name)
    a = r["a"]
    payloads = [ac.state_dict(layout, wf[c % a], wi[c % a]) for c in range(a + extra)]
    rnd = engine.begin(payloads[0], a + extra)
    rnd.deltas = False
    rnd.put_baseline(ac.state_dict(layout, bf, bi))
    for slot, p in enumerate(payloads):
        rnd.put_client(slot, p)
    rnd.launch_attack(r["kind"], range(a), **{k: r[k] for k in ("per_round", "lambada_value") if k in r})
    fetched = rnd.fetch_rows(range(a + extra))
    out_f = np.stack([f.numpy() for f, _ in fetched])
    out_i = np.stack([i.numpy() for _, i in fetched])
    info = dict(rnd.attack)
    if info["poisoned"]:
        info["vector"] = np.concatenate([t.cpu().numpy() for t in info["vector"]])
    return out_f, out_i, info, rnd


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith(("lie", "lambda"))])
def test_lie_and_lambda_against_the_reference(engine, name):
    case = case_of(name)
    r, exp = case["recipe"], case["expected"]
    _, bf, bi, wf, wi, u = inputs(name)
    a = r["a"]
    out_f, out_i, info, rnd = run_attack(engine, name, extra=1)
    # the row behind the attackers is no attacker's: untouched
    assert np.array_equal(bits(out_f[a]), bits(wf[0])) and np.array_equal(out_i[a], wi[0])
    digests = [ac.row_digest(out_f[c], out_i[c]) for c in range(a)]
    if r["kind"] == "lie" or a <= 4:  # the Welford std is exact at every A; torch.mean is sequential up to 4
        assert digests == exp["rows"]
        if info["poisoned"]:
            assert ac.sha(ac.canon(info["vector"])) == exp["sha_vector"]
            assert rnd.timings["add_scaled_rows_ms"] > 0
        return
    # Lambda from A = 5 up: by parts
    idx, ref = ac.sampled(exp["samples_vector"])
    bound = ko.mean_bound(u, range(a), info["vector"])
    err = np.abs(info["vector"][idx].astype(np.float64) - ref)
    assert np.all(err <= bound[idx])
    full = ac.load_full()
    if name + ".vector" in full.files:
        ref_all = full[name + ".vector"]
        assert np.all(np.abs(info["vector"].astype(np.float64) - ref_all) <= bound)
    assert same(info["vector"], ao.mean(u))
    exp_f, exp_i, _ = ao.attack("lambda", wf, wi, bf, bi, lambada_value=r["lambada_value"], vector=info["vector"])
    assert np.array_equal(bits(out_f[:a]), bits(exp_f)) and np.array_equal(out_i[:a], exp_i)
    print(f"{name}: max |mean - mean_ref| / bound = {float(np.max(err / bound[idx])):.4f}")


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith(("minmax", "minsum"))])
def test_min_max_and_min_sum_against_the_reference(engine, name):
    case = case_of(name)
    r, exp = case["recipe"], case["expected"]
    kind, a = r["kind"], r["a"]
    _, bf, bi, wf, wi, u = inputs(name)
    out_f, out_i, info, rnd = run_attack(engine, name)
    lam, norm = info["lam"], info["norm"]
    lam_ref, lo, hi = (ac.hexf(exp[k]) for k in ("lambda_ref", "lambda_lo", "lambda_hi"))
    print(f"{name}: lambda {float(lam)!r} (reference {float(lam_ref)!r}, interval [{float(lo)!r}, {float(hi)!r}])")
    # 1. the device's lambda lies in the float64 interval
    assert lam.dtype == np.float32 and lo <= lam <= hi
    # 2. the device's norm within 1 ulp (fp32) of the oracle's float64 norm of the device's own average
    cols = ao.columns(wf, wi) if kind == "minsum" else u
    avg = ao.mean(cols)
    n64 = ao.norm64(avg)
    assert norm.dtype == np.float32 and abs(float(norm) - n64) <= float(np.spacing(np.float32(n64)))
    # 3. the poisoned rows equal the restatement evaluated with the device's lambda and norm, bit for bit
    exp_f, exp_i, mine = ao.attack(kind, wf, wi, bf, bi, lam=lam, norm=norm)
    assert same(info["vector"], mine["vector"])
    assert np.array_equal(bits(out_f), bits(exp_f)) and np.array_equal(out_i, exp_i)
    assert bits(info["s"]) == bits(mine["s"])
    # 4. against the reference's poisoned payload of attacker 0, on the sampled elements, the issue's three
    # terms: |lam_dev - lam_ref| |p_e|, the propagated mean bound, 2 ulp.  The mean bound propagates through
    # p = avg / |avg|: by mean_bound_e / |avg| in the numerator and by |p_e| times the norms' relative gap,
    # the recorded one (the device's norm against the reference's), in the denominator.  The ulp is that of
    # the largest of the weight, the poison and the result (the product and the sum are rounded once each).
    n_f = wf.shape[1]
    idx, ref_row0 = ac.sampled(exp["samples_row0"])
    _, ref_poison = ac.sampled(exp["samples_poison"])
    p = info["vector"].astype(np.float64)
    mean_bound = ko.mean_bound(cols, range(a), avg)
    norm_gap = abs(float(norm) - float(ac.hexf(exp["norm_ref"]))) / n64
    p_bound = mean_bound / n64 + np.abs(p) * norm_gap
    poison = (np.float32(info["s"]) * info["vector"]).astype(np.float32)
    row0 = np.concatenate([wf[0], wi[0].astype(np.float32)])
    got_row0 = np.concatenate([out_f[0], out_i[0].astype(np.float32)])
    biggest = np.maximum(np.maximum(np.abs(ref_row0), np.abs(row0[idx])), np.abs(poison[idx]))
    ulp = np.spacing(biggest.astype(np.float32)).astype(np.float64)
    lam64 = max(float(lam), float(lam_ref))
    bound = abs(float(lam) - float(lam_ref)) * np.abs(p[idx]) + lam64 * p_bound[idx] + 2 * ulp
    err = np.abs(got_row0[idx].astype(np.float64) - ref_row0.astype(np.float64))
    # the counters take the truncated poison: the poisons themselves within the bound, and a step of one only
    # where an integer lies between the device's poison and the reference's
    counter = idx >= n_f
    poison_err = np.abs(poison[idx].astype(np.float64) - ref_poison.astype(np.float64))
    assert np.all(poison_err[counter] <= bound[counter])
    crossed = np.trunc(poison[idx].astype(np.float64)) != np.trunc(ref_poison.astype(np.float64))
    bound = np.where(counter, crossed.astype(np.float64), bound)
    ratio = np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)
    print(f"{name}: max |row - row_ref| = {float(err.max()):.3e}, max err / bound = {float(ratio.max()):.4f}, "
          f"|lam - lam_ref| = {abs(float(lam) - float(lam_ref)):.3e}, norm gap = {norm_gap:.3e}, "
          f"max |poison - poison_ref| = {float(poison_err.max()):.3e}")
    assert np.all(err <= bound)
    t = rnd.timings
    assert t["pairwise_sqdist_ms"] > 0 and t["attack_stats_ms"] > 0 and t["attack_search_ms"] >= 0


def test_identical_attackers_are_poisoned_with_a_zero_vector(engine):
    layout, bf, bi, wf, wi, _ = inputs("minmax_bn_toy_a3")
    payloads = [ac.state_dict(layout, wf[0], wi[0]) for _ in range(3)]
    rnd = engine.begin(payloads[0], 3)
    rnd.deltas = False
    rnd.put_baseline(ac.state_dict(layout, bf, bi))
    for slot, p in enumerate(payloads):
        rnd.put_client(slot, p)
    rnd.launch_attack("minmax", range(3))
    assert rnd.attack["threshold"] == 0 and rnd.attack["lam"] == 0
    for f, i in rnd.fetch_rows(range(3)):
        assert np.array_equal(f.numpy(), wf[0]) and np.array_equal(i.numpy(), wi[0])


def test_refusals(engine):
    layout, bf, bi, wf, wi, _ = inputs("lie_bn_toy_a3_n100")
    payloads = [ac.state_dict(layout, wf[c], wi[c]) for c in range(3)]
    rnd = engine.begin(payloads[0], 3)
    rnd.deltas = False
    for slot, p in enumerate(payloads):
        rnd.put_client(slot, p)
    with pytest.raises(ValueError, match="stage the baseline"):
        rnd.launch_attack("lie", range(3), per_round=100)
    rnd.put_baseline(ac.state_dict(layout, bf, bi))
    with pytest.raises(ValueError, match="unknown attack"):
        rnd.launch_attack("Fang", range(3))
    with pytest.raises(ValueError, match="per_round"):
        rnd.launch_attack("lie", range(3))
    with pytest.raises(ValueError, match="lambada_value"):
        rnd.launch_attack("lambda", range(3))
    with pytest.raises(ValueError, match="no client slots"):
        rnd.launch_attack("minmax", [])
    a = 1 << 12  # any aligned non-null address: nothing is dereferenced on these paths
    for m in (0, 257):
        with pytest.raises(ValueError, match="m must be in 1..256"):
            _lib.call("plato_agg_column_std", a, None, m, a, None, 16, 0, None)
        with pytest.raises(ValueError, match="m must be in 1..256"):
            _lib.call("plato_agg_add_scaled_rows", a, None, m, 1.0, a, None, 16, 0, None)
    with pytest.raises(ValueError, match="null"):
        _lib.call("plato_agg_column_std", a, None, 2, None, None, 16, 0, None)
    with pytest.raises(ValueError, match="null int64"):
        _lib.call("plato_agg_add_scaled_rows", a, None, 2, 1.0, a, None, 16, 1, None)
    with pytest.raises(ValueError, match="16-byte aligned"):
        _lib.call("plato_agg_column_std", a, None, 2, a + 4, None, 16, 0, None)
    assert _lib.lib().plato_agg_column_std(None, None, 2, None, None, 0, 0, None) == _lib.PLATO_AGG_OK


# ------------------------------------------------------------------ the server hook
class _Base:
    """What the hooks need of the detector server."""

    base_calls = 0

    def weights_attacked(self, weights_received):
        self.base_calls += 1
        return weights_received


class _Mixin(AttackSimulationMixin, DetectorAggregationMixin):
    pass


def _server(name, attack_type, attackers, **settings):
    import asyncio

    r = case_of(name)["recipe"]
    layout, bf, bi, wf, wi, _ = inputs(name)
    server = make_server(base=_Base, mixin=_Mixin)()
    server.aggregation_device = "cuda:0"
    server.secure_aggregation_type = "Median"
    server.attack_simulation_type = attack_type
    server.attack_per_round = r.get("per_round")
    for key, value in settings.items():
        setattr(server, key, value)
    k = r["a"] + 2  # two benign clients around the attackers
    ids = list(range(1, k + 1))
    server.attacker_list = [ids[c] for c in attackers]
    server.updates = [types.SimpleNamespace(client_id=i, report=types.SimpleNamespace(num_samples=10)) for i in ids]
    server.algorithm = types.SimpleNamespace(extract_weights=lambda: ac.state_dict(layout, bf, bi))
    a = r["a"]
    payloads = [ac.state_dict(layout, wf[c], wi[c]) for c in [a - 1, *range(a), 0]]  # clients 2..a+1 in case order
    return server, payloads, lambda p: asyncio.run(server.aggregate_weights(server.updates, None, p))


def _flat(layout, payloads):
    flat = [ac.flat_payload(layout, p) for p in payloads]
    return np.stack([f for f, _ in flat]), np.stack([i for _, i in flat])


@pytest.mark.parametrize("writeback", (True, False))
@pytest.mark.parametrize("name", ("lie_lenet5_a3_n100", "lie_bn_toy_a3_n100"))  # 61 tiles; and the counters
def test_server_runs_lie_then_median_and_the_next_round_uses_the_payloads(name, writeback):
    layout, bf, bi, wf, wi, _ = inputs(name)
    server, payloads, aggregate = _server(name, "LIE", (1, 2, 3), attack_writeback=writeback)
    xf, xi = _flat(layout, payloads)
    for rounds in range(2):
        before = [t._version for t in payloads[1].values()]
        out = server.weights_attacked(payloads)
        assert out is payloads and server.base_calls == 0
        pf, pi, _ = ao.attack("lie", xf[1:4], xi[1:4], bf, bi, per_round=100)
        exp_f, exp_i = xf.copy(), xi.copy()
        exp_f[1:4], exp_i[1:4] = pf, pi
        got_f, got_i = _flat(layout, payloads)
        if writeback:  # the payload tensors were written in place, as the reference writes them
            assert np.array_equal(bits(got_f), bits(exp_f)) and np.array_equal(got_i, exp_i)
            assert [t._version for t in payloads[1].values()] != before
        else:
            assert np.array_equal(bits(got_f), bits(xf)) and np.array_equal(got_i, xi)
        staged = server.aggregation_engine()._arrivals.free_count()
        result = aggregate(payloads)
        # the aggregator saw the poisoned rows, and adopted the attackers' rows where they lay
        got = np.concatenate([result[e.name].reshape(-1).numpy() for reg in ("f32", "i64")
                              for e in layout.entries if e.region == reg])
        exp_median = np.sort(ao.columns(exp_f, exp_i), axis=0)[(exp_f.shape[0] - 1) // 2]
        assert np.array_equal(bits(got), bits(exp_median))
        assert server.aggregation_engine()._arrivals.free_count() == staged + 3  # released after the round
        assert server._plato_amd_attack["kind"] == "lie" and server._plato_amd_attack["poisoned"]
        if not writeback:
            break  # the payloads still hold the clean weights: a second round would repeat the first
        xf, xi = exp_f, exp_i  # the next round starts from the written-back payloads


def test_server_leaves_payloads_alone_without_attackers_and_for_a_solo_lie():
    name = "lie_bn_toy_a3_n100"
    layout = inputs(name)[0]
    for attackers in ((), (2,)):
        server, payloads, _ = _server(name, "LIE", attackers)
        xf, xi = _flat(layout, payloads)
        versions = [[t._version for t in p.values()] for p in payloads]
        assert server.weights_attacked(payloads) is payloads and server.base_calls == 0
        got_f, got_i = _flat(layout, payloads)
        assert np.array_equal(bits(got_f), bits(xf)) and np.array_equal(got_i, xi)
        assert versions == [[t._version for t in p.values()] for p in payloads]


@pytest.mark.parametrize("attack_type", ("Fang", "Gassian_attack", "Oblivion-lie", None))
def test_server_sends_every_other_attack_to_the_base_class(attack_type):
    server, payloads, _ = _server("lie_bn_toy_a3_n100", attack_type, (1, 2, 3))
    assert server.weights_attacked(payloads) is payloads and server.base_calls == 1
    assert getattr(server, "_plato_amd_engine", None) is None  # nothing was staged


@pytest.mark.parametrize("name", ("minmax_bn_toy_a3", "minsum_bn_toy_a3", "lambda_bn_toy_a3"))
def test_server_runs_the_other_attacks(name):
    r = case_of(name)["recipe"]
    layout, bf, bi, wf, wi, _ = inputs(name)
    server, payloads, _ = _server(name, ac.ATTACK_TYPE[r["kind"]], (1, 2, 3), attack_lambada_value=ac.LAMBADA)
    server.weights_attacked(payloads)
    got_f, got_i = _flat(layout, payloads)
    digests = [ac.row_digest(got_f[c], got_i[c]) for c in (1, 2, 3)]
    info = server._plato_amd_attack
    if r["kind"] == "lambda":
        assert digests == case_of(name)["expected"]["rows"]
    else:
        exp_f, exp_i, _ = ao.attack(r["kind"], wf, wi, bf, bi, lam=info["lam"], norm=info["norm"])
        lo, hi = (ac.hexf(case_of(name)["expected"][k]) for k in ("lambda_lo", "lambda_hi"))
        assert lo <= info["lam"] <= hi
        assert np.array_equal(bits(got_f[1:4]), bits(exp_f)) and np.array_equal(got_i[1:4], exp_i)
    assert np.array_equal(bits(got_f[0]), bits(wf[2])) and np.array_equal(bits(got_f[4]), bits(wf[0]))


def test_every_case_is_covered():
    assert len(CASES) == 25 and sum(n.startswith("lie") for n in NAMES) == 10
