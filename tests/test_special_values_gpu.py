"""The variant servers' reduction kernels at non-finite, overflowing and tiny values.

tests/special_values.py builds the cases; tests/test_reductions.py pins the C restatements
(oracle/reductions.c) to torch and numpy on them, on the CPU.  Here the device kernels must equal the
restatements bit for bit on the same inputs (a NaN matches any NaN: the device's default NaN is positive,
x86's negative), in every kernel variant, on weight arenas and on delta arenas; and one poisoned (client,
entry) must change no output that does not read it.

Outputs that go through the C ABI are sentinel-filled with guard words behind them (tests/edge_cases.py).
"""

import numpy as np
import pytest
import torch

from oracle import fedavg_oracle as FO
from oracle import reductions as R
from plato_amd import _lib
from plato_amd.engine import FedAvgEngine
from tests import edge_cases as EC
from tests import special_values as SV

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-8


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _take32(t, n: int) -> np.ndarray:
    """The n floats of a guarded output; the guard behind them must be untouched."""
    torch.cuda.synchronize()
    a = EC.fetch(t, np.uint32)
    assert (a[n:] == EC.SENTINEL32).all(), "guard words behind the output overwritten"
    return a[:n].view(np.float32).copy()


def _check(got, want, what, by_value=False):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, what
    ok = (np.isnan(got) & np.isnan(want)) | ((got == want) if by_value else (got.view(np.uint32) == want.view(np.uint32)))
    if not ok.all():
        bad = np.argwhere(~ok)
        rows = [(tuple(int(x) for x in i), got[tuple(i)].view(np.uint32).item(), want[tuple(i)].view(np.uint32).item(),
                 float(got[tuple(i)]), float(want[tuple(i)])) for i in bad[:8]]
        raise AssertionError(f"{what}: {len(bad)} differ; (index, got bits, want bits, got, want): "
                             + "; ".join(f"{i} {g:08x} {w:08x} {gf!r} {wf!r}" for i, g, w, gf, wf in rows))


def _rows(vecs):
    """[len, stride] device buffer (64-float aligned rows, NaN behind each vector) and its row pointers."""
    n = max(v.size for v in vecs)
    stride = max(64, -(-n // 64) * 64)
    host = np.full((len(vecs), stride), np.nan, np.float32)
    for r, v in enumerate(vecs):
        host[r, : v.size] = v
    buf = torch.from_numpy(host).to(DEV)
    ptrs = torch.tensor([buf.data_ptr() + r * stride * 4 for r in range(len(vecs))], dtype=torch.int64, device=DEV)
    return buf, ptrs


class Staged:
    """A case's arenas on the device, as weights (with the baseline) or as deltas (null baseline); the
    floats between n_f32 and the row's end hold NaN (read by clamped loads, never summed)."""

    def __init__(self, case, deltas: bool):
        lay, k = case["layout"], case["k"]
        xs_f, xs_i = SV.arena_deltas(case) if deltas else (case["xs_f"], case["xs_i"])
        host = np.full((k, lay.row_f32), np.nan, np.float32)
        host[:, : lay.n_f32] = xs_f
        self.xf = torch.from_numpy(host).to(DEV)
        self.xi = torch.from_numpy(np.ascontiguousarray(xs_i)).to(DEV)
        self.pf = [self.xf[i].data_ptr() for i in range(k)]
        self.pi = [self.xi[i].data_ptr() for i in range(k)]
        self.tf = torch.tensor(self.pf, dtype=torch.int64, device=DEV)
        self.ti = torch.tensor(self.pi, dtype=torch.int64, device=DEV)
        hb = np.full(lay.row_f32, np.nan, np.float32)
        hb[: lay.n_f32] = case["bf"]
        self._bf, self._bi = torch.from_numpy(hb).to(DEV), torch.from_numpy(case["bi"]).to(DEV)
        self.bf = None if deltas else self._bf.data_ptr()
        self.bi = None if deltas else self._bi.data_ptr()


def _arena_cases(lay, k, one_per_client=False, rotations=range(len(SV.SINGLE))):
    """(label, case): ordinary data with the wrapping counters, every WHOLE class over the whole arena,
    a WHOLE class per (client, entry) in turn, and every SINGLE class on every spot."""
    yield "clean", SV.arena_case(lay, k)
    for cls in SV.WHOLE:
        yield cls, SV.arena_case(lay, k, cls)
    f32 = [e.name for e in lay.entries if e.region == "f32"]
    yield "whole per entry", SV.arena_case(lay, k, targets=[(j % k, n, "first", SV.WHOLE[j % 5])
                                                            for j, n in enumerate(f32)])
    for r in rotations:
        for g, targets in enumerate(SV.spot_groups(lay, k, r, one_per_client)):
            yield f"spots r{r} g{g}", SV.arena_case(lay, k, seed=r, targets=targets)


# ------------------------------------------------------------------------------------------------
# plato_agg_entry_norms_f32
# ------------------------------------------------------------------------------------------------
def _norm_tables(lay):
    ef, ei = lay.chunk_tables(1 << 32)
    ef = ef[np.argsort(-(ef[:, 2].astype(np.int64) - ef[:, 1]), kind="stable")]
    return (torch.from_numpy(np.ascontiguousarray(ef).view(np.int32).copy()).to(DEV),
            torch.from_numpy(np.ascontiguousarray(ei).view(np.int32).copy()).to(DEV))


def _want_norms(case) -> np.ndarray:
    lay = case["layout"]
    d_f, d_i = SV.arena_deltas(case)
    d_i = d_i.astype(np.float32)
    want = np.zeros((case["k"], len(lay.entries)), np.float32)
    for e_i, e in enumerate(lay.entries):
        src = d_f if e.region == "f32" else d_i
        for c in range(case["k"]):
            want[c, e_i] = R.torch_norm(src[c, e.offset:e.offset + e.numel])
    return want


def _entry_norms(st, lay, k, tabs, variant=None) -> np.ndarray:
    n_e = len(lay.entries)
    out = EC.guarded(k * n_e, EC.SENTINEL32, DEV)
    args = (st.tf.data_ptr(), st.ti.data_ptr(), k, st.bf, st.bi, tabs[0].data_ptr(), tabs[0].shape[0],
            tabs[1].data_ptr(), tabs[1].shape[0], n_e, lay.n_f32, lay.n_i64, out.data_ptr(), _stream())
    if variant is None:
        _lib.call("plato_agg_entry_norms_f32", *args)
    else:
        _lib.tune_call("plato_agg_tune_entry_norms", variant, *args)
    return _take32(out, k * n_e).reshape(k, n_e)


@pytest.mark.parametrize("deltas", [False, True], ids=["weight_arenas", "delta_arenas"])
@pytest.mark.parametrize("k", [1, 3, 5, 97, 128, 129])
def test_entry_norms_at_special_values(k, deltas):
    """Every entry_norms kernel == torch.linalg.norm's bits per (client, entry): one client per workgroup
    (K <= 5), two and four folded into one chain wave (97; 128, 129, on the entries up to (257,)), scalar
    entries (|d|, no square), int64 entries whose squares overflow."""
    lay = SV.layout(small=k > 5)
    tabs = _norm_tables(lay)
    variants = [None] + list(range(_lib.tune().plato_agg_tune_num_entry_norms_variants()))
    rotations = range(len(SV.SINGLE)) if k <= 5 else (0, 3)
    for label, case in _arena_cases(lay, k, rotations=rotations):
        st, want = Staged(case, deltas), _want_norms(case)
        for v in variants:
            _check(_entry_norms(st, lay, k, tabs, v), want, f"entry_norms {label} variant {v} [client, entry]")


# ------------------------------------------------------------------------------------------------
# plato_agg_port_norms
# ------------------------------------------------------------------------------------------------
def _segments(lay):
    rows, flat = [], 0
    for e in lay.entries:
        rows.append([flat, e.offset, e.numel, 0 if e.region == "f32" else 1])
        flat += e.numel
    return torch.from_numpy(np.asarray(rows, dtype=np.uint64).view(np.int64)).to(DEV), flat


def _port_vectors(case, cast_first: bool):
    """Vector 0: current (the baseline) minus previous (the case's last client); vectors 1..k-1: the other
    clients' deltas against the baseline."""
    ents, k = case["layout"].entries, case["k"]
    with np.errstate(all="ignore"):
        if cast_first:
            v0 = R.port_current_minus_previous(ents, case["bf"], case["bi"], case["xs_f"][k - 1], case["xs_i"][k - 1])
        else:
            v0 = R.port_delta(ents, case["xs_f"][k - 1], case["xs_i"][k - 1], case["bf"], case["bi"])
        return [v0] + [R.port_delta(ents, case["bf"], case["bi"], case["xs_f"][c], case["xs_i"][c]) for c in range(k - 1)]


@pytest.mark.parametrize("cast_first", [False, True], ids=["cast_once", "cast_first"])
@pytest.mark.parametrize("deltas", [False, True], ids=["weight_arenas", "delta_arenas"])
def test_port_norms_at_special_values(deltas, cast_first):
    """plato_agg_port_norms (the default and every variant; flat rows stored or not; whole vectors and
    per-vector lengths 1, 8, 8193) == torch's vector_norm of the flattened differences, and the stored rows
    == those vectors, with nothing written behind a vector's length."""
    lay = SV.layout()
    segs, n_flat = _segments(lay)
    k = 5  # vectors: current - previous, 4 clients
    lens = np.asarray([n_flat, 1, 8, 8193, 25373 + 6], dtype=np.uint32)  # the last: up to the end of v8193
    d_lens = torch.from_numpy(lens.view(np.int32)).to(DEV)
    stride = -(-n_flat // 64) * 64
    variants = [None] + list(range(_lib.tune().plato_agg_tune_num_port_norms_variants()))
    for label, case in _arena_cases(lay, k, one_per_client=True):
        vecs = _port_vectors(case, cast_first)
        if deltas:  # the clients' arenas hold x - b already (null subtrahend); vector 0 keeps both operands
            d_f, d_i = SV.arena_deltas(case)
            d_f[k - 1], d_i[k - 1] = case["xs_f"][k - 1], case["xs_i"][k - 1]  # the previous model stays a model
            case_x = dict(case, xs_f=d_f, xs_i=d_i)
        else:
            case_x = case
        st = Staged(case_x, False)
        xf = [st._bf.data_ptr()] + st.pf[: k - 1]
        xi = [st._bi.data_ptr()] + st.pi[: k - 1]
        bf = [st.pf[k - 1]] + [0 if deltas else st._bf.data_ptr()] * (k - 1)
        bi = [st.pi[k - 1]] + [0 if deltas else st._bi.data_ptr()] * (k - 1)
        want_rows = np.full((k, stride), np.nan, np.float32)
        for v, vec in enumerate(vecs):
            want_rows[v, :n_flat] = vec
        for use_len in (False, True):
            want_n = np.asarray([R.torch_norm(vec[: int(lens[v])] if use_len else vec) for v, vec in enumerate(vecs)])
            for with_flat in (False, True):
                flat = EC.guarded(k * stride, EC.SENTINEL32, DEV)
                tab = torch.tensor(xf + xi + bf + bi + [flat.data_ptr() + 4 * stride * r for r in range(k)],
                                   dtype=torch.int64, device=DEV)
                p = tab.data_ptr()
                for variant in variants:
                    out = EC.guarded(k, EC.SENTINEL32, DEV)
                    args = (p, p + 8 * k, p + 16 * k, p + 24 * k, k, d_lens.data_ptr() if use_len else None,
                            segs.data_ptr(), len(lay.entries), n_flat, lay.n_f32,
                            _lib.PLATO_AGG_PORT_CAST_FIRST if cast_first else 0, out.data_ptr(),
                            p + 32 * k if with_flat else None, _stream())
                    if variant is None:
                        _lib.call("plato_agg_port_norms", *args)
                    else:
                        _lib.tune_call("plato_agg_tune_port_norms", variant, *args)
                    what = f"port_norms {label} variant {variant} lengths {use_len} flat {with_flat}"
                    _check(_take32(out, k), want_n, what + " [vector]")
                    rows = _take32(flat, k * stride).reshape(k, stride)
                    for v in range(k):
                        ln = (int(lens[v]) if use_len else n_flat) if with_flat else 0
                        _check(rows[v, :ln], want_rows[v, :ln], what + f" flat row {v}")
                        assert (rows[v, ln:].view(np.uint32) == EC.SENTINEL32).all(), what + f": row {v} written past {ln}"
                    if with_flat:
                        flat.copy_(EC.guarded(k * stride, EC.SENTINEL32, DEV))


# ------------------------------------------------------------------------------------------------
# plato_agg_scale_by_norm, plato_agg_torch_cosine_sum, plato_agg_torch_cosine_sum_scaled
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("n", [1, 2, 9, 1000, 32773, 65541])
def test_cosine_sums_at_special_values(n, threads):
    """max(norm, eps) with a norm of 0, below, at and above eps, inf and NaN; quotients of subnormals and of
    values near FLT_MAX; NaN and +-inf through the cascade sum (one pass and two).  The norms are the
    restatement's, uploaded: a departure here is the cosine kernels' own."""
    n_var = _lib.tune().plato_agg_tune_num_cosine_variants()
    ws = torch.empty(_lib.lib().plato_agg_torch_cosine_workspace(2, threads) // 4 + 1, device=DEV)
    h = _stream()
    for cls, p, a, b in SV.vector_cases(n):
        what = f"{cls} at {p}, n {n}, threads {threads}"
        bs = [b, a]
        with np.errstate(all="ignore"):
            norms = np.asarray([R.torch_norm(a), R.torch_norm(b), R.torch_norm(a)], np.float32)
            want = np.asarray([R.torch_cosine(a, y, threads) for y in bs])
            na = norms[0] if not norms[0] < SV.EPS else SV.EPS
            want_scaled = np.divide(a, na, dtype=np.float32)
        buf, ptrs = _rows([a] + bs)
        d_norms = torch.from_numpy(norms).to(DEV)
        out = EC.guarded(2, EC.SENTINEL32, DEV)
        _lib.call("plato_agg_torch_cosine_sum", buf.data_ptr(), ptrs.data_ptr() + 8, 2, n, d_norms.data_ptr(),
                  d_norms.data_ptr() + 4, EPS, threads, ws.data_ptr(), out.data_ptr(), h)
        _check(_take32(out, 2), want, "cosine_sum " + what)
        scaled = EC.guarded(n, EC.SENTINEL32, DEV)
        _lib.call("plato_agg_scale_by_norm", buf.data_ptr(), n, d_norms.data_ptr(), EPS, scaled.data_ptr(), h)
        _check(_take32(scaled, n), want_scaled, "scale_by_norm " + what)
        for v in [None] + list(range(n_var)):
            out = EC.guarded(2, EC.SENTINEL32, DEV)
            args = (scaled.data_ptr(), ptrs.data_ptr() + 8, 2, n, d_norms.data_ptr() + 4, EPS, threads, ws.data_ptr(),
                    out.data_ptr(), h)
            if v is None:
                _lib.call("plato_agg_torch_cosine_sum_scaled", *args)
            else:
                _lib.tune_call("plato_agg_tune_torch_cosine_sum_scaled", v, *args)
            _check(_take32(out, 2), want, f"cosine_sum_scaled variant {v} " + what)


# ------------------------------------------------------------------------------------------------
# plato_agg_sdot_pairs, plato_agg_sdot_shared
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npairs", [3, 9])
@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 63, 64, 65, 4097, 8193])
def test_sdot_at_special_values(n, npairs):
    """OpenBLAS' sdot order with special values in the 64- and 32-element blocks and in the float64 tail.
    n = 1 is compared by value: the kernels return +0 + product where np.inner returns the bare product
    (-0 against +0), which FedAdp's arccos(inner / norms) cannot tell apart (include/plato_agg.h)."""
    cases = list(SV.vector_cases(n))
    cases += cases[: (-len(cases)) % npairs]  # whole batches
    n_var = _lib.tune().plato_agg_tune_num_sdot_shared_variants()
    ws = torch.empty(_lib.lib().plato_agg_sdot_shared_workspace(npairs, 1) // 4, dtype=torch.float32, device=DEV)
    h = _stream()
    for s0 in range(0, len(cases), npairs):
        batch = cases[s0:s0 + npairs]
        what = f"n {n}, cases {[(c[0], c[1]) for c in batch]}"
        xs, ys = [c[2] for c in batch], [c[3] for c in batch]
        with np.errstate(all="ignore"):
            want_xy = np.asarray([R.sdot(x, y) for x, y in zip(xs, ys)])
            want_yy = np.asarray([R.sdot(y, y) for y in ys])
        bx, px = _rows(xs)
        by, py = _rows(ys)
        o_xy, o_yy = EC.guarded(npairs, EC.SENTINEL32, DEV), EC.guarded(npairs, EC.SENTINEL32, DEV)
        _lib.call("plato_agg_sdot_pairs", px.data_ptr(), py.data_ptr(), npairs, n, o_xy.data_ptr(), o_yy.data_ptr(), h)
        _check(_take32(o_xy, npairs), want_xy, "sdot_pairs xy " + what, by_value=n == 1)
        _check(_take32(o_yy, npairs), want_yy, "sdot_pairs yy " + what, by_value=n == 1)
        # the shared-x kernels: x = the batch's first a (and then its first b) against every y
        for x in (xs[0], ys[-1]):
            with np.errstate(all="ignore"):
                xx = R.sdot(x, x)
                s_xy = np.asarray([R.sdot(x, y) for y in ys] + [xx])
                s_yy = np.append(want_yy, xx)
            bx1, _ = _rows([x])
            for v in [None] + list(range(n_var)):
                for with_xx in (0, 1):
                    o_xy = EC.guarded(npairs + with_xx, EC.SENTINEL32, DEV)
                    o_yy = EC.guarded(npairs + with_xx, EC.SENTINEL32, DEV)
                    args = (bx1.data_ptr(), py.data_ptr(), npairs, n, with_xx, ws.data_ptr(), o_xy.data_ptr(),
                            o_yy.data_ptr(), h)
                    if v is None:
                        _lib.call("plato_agg_sdot_shared", *args)
                    else:
                        _lib.tune_call("plato_agg_tune_sdot_shared", v, *args)
                    m = npairs + with_xx
                    _check(_take32(o_xy, m), s_xy[:m], f"sdot_shared variant {v} xx {with_xx} xy " + what, by_value=n == 1)
                    _check(_take32(o_yy, m), s_yy[:m], f"sdot_shared variant {v} xx {with_xx} yy " + what, by_value=n == 1)


# ------------------------------------------------------------------------------------------------
# plato_agg_np_sumsq
# ------------------------------------------------------------------------------------------------
def _sumsq_tables(lay):
    rows, first, n_chunks = [], [], 0
    for idx, e in enumerate(lay.entries):
        if e.region == "f32" and e.numel:
            rows.append((idx, e.offset, e.offset + e.numel, 0))
            first.append(n_chunks)
            n_chunks += -(-e.numel // 8192)
    pieces = np.asarray(rows, dtype=np.uint32).reshape(-1, 4)
    return (torch.from_numpy(pieces.view(np.int32).copy()).to(DEV),
            torch.from_numpy(np.asarray(first, dtype=np.uint32).view(np.int32)).to(DEV), pieces[:, 0].astype(np.int64),
            n_chunks)


def _np_sumsq(st, k, tables, variant=None) -> np.ndarray:
    pieces, first, entry_of, n_chunks = tables
    n_p = int(entry_of.size)
    ws = torch.full((max(1, _lib.lib().plato_agg_np_sumsq_workspace(k, n_chunks) // 4),), float("nan"), device=DEV)
    out = EC.guarded(k * n_p, EC.SENTINEL32, DEV)
    args = (st.tf.data_ptr(), k, st.bf, pieces.data_ptr(), first.data_ptr(), n_p, n_chunks, ws.data_ptr(),
            out.data_ptr(), _stream())
    if variant is None:
        _lib.call("plato_agg_np_sumsq", *args)
    else:
        _lib.tune_call("plato_agg_tune_np_sumsq", variant, *args)
    return _take32(out, k * n_p).reshape(k, n_p)


NP_SUMSQ_PROBES = (2, 3)  # timing probes: wrong results by design (tests/test_flat_gpu.py)
NP_SUMSQ_DELTA_VARIANTS = (0, 6, 14)  # the kernels that take a null baseline (tests/test_flat_gpu.py)


@pytest.mark.parametrize("deltas", [False, True], ids=["weight_arenas", "delta_arenas"])
def test_np_sumsq_at_special_values(deltas):
    """numpy's pairwise float32 sum of squares per (client, fp32 entry), two to four clients per
    workgroup (K = 5: ragged last groups), every kernel that is not a timing probe."""
    lay, k = SV.layout(), 5
    tables = _sumsq_tables(lay)
    every = [v for v in range(_lib.tune().plato_agg_tune_num_np_sumsq_variants()) if v not in NP_SUMSQ_PROBES]
    variants = [None] + (list(NP_SUMSQ_DELTA_VARIANTS) if deltas else every)
    for label, case in _arena_cases(lay, k):
        d_f, _ = SV.arena_deltas(case)
        with np.errstate(all="ignore"):
            want = np.asarray([[R.np_sum(np.square(d_f[c, e.offset:e.offset + e.numel])) for e in lay.entries
                                if e.region == "f32"] for c in range(k)])
        st = Staged(case, deltas)
        for v in variants:
            _check(_np_sumsq(st, k, tables, v), want, f"np_sumsq {label} variant {v} [client, piece]")


# ------------------------------------------------------------------------------------------------
# the engine's FedAdp dots and entrywise sums
# ------------------------------------------------------------------------------------------------
def _staged_round(engine, case):
    lay, k = case["layout"], case["k"]
    base = lay.unpack(torch.from_numpy(case["bf"]), torch.from_numpy(case["bi"]))
    rnd = engine.begin(base, k)
    rnd.put_baseline(base)
    for c in range(k):
        rnd.put_client(c, lay.unpack(torch.from_numpy(case["xs_f"][c]), torch.from_numpy(case["xs_i"][c])))
    return rnd


def _fedadp_gradient(case, seed):
    """A global gradient arena: ordinary numbers, the case's class where it has one, +inf where a client
    holds -inf (pm_inf: the product is -inf, two of them in one dot would be NaN)."""
    lay = case["layout"]
    rng = np.random.default_rng([11, seed])
    gf = (rng.standard_normal(lay.n_f32) * 0.01).astype(np.float32)
    if case["cls"] is not None:
        gf = SV.whole_values(case["cls"], lay.n_f32, rng)
    for (_, _, _, kind), at in zip(case["targets"], case["at"]):
        if kind == "pm_inf":
            gf[at] = np.inf
    return gf, rng.standard_normal(lay.n_i64).astype(np.float32)


def _fedadp_want(case, gf, gi, lr):
    lay, k = case["layout"], case["k"]
    d_f, d_i = SV.arena_deltas(case)
    with np.errstate(all="ignore"):
        g = FO.fedadp_flatten({n: t.numpy() for n, t in lay.unpack(torch.from_numpy(gf), torch.from_numpy(gi)).items()}, lr)
        locs = [FO.fedadp_flatten(lay.unpack(torch.from_numpy(d_f[c]), torch.from_numpy(d_i[c])), lr) for c in range(k)]
        assert g.dtype == np.float32 and all(v.dtype == np.float32 and v.size == g.size for v in locs)
        return (np.asarray([R.sdot(g, v) for v in locs]), R.sdot(g, g), np.asarray([R.sdot(v, v) for v in locs]))


@pytest.mark.parametrize("lr", [0.03, 98.0])
@pytest.mark.parametrize("deltas", [False, True], ids=["weight_arenas", "delta_arenas"])
def test_fedadp_dots_at_special_values(deltas, lr):
    """rnd.fedadp_dots == numpy's sdot of process_grad's flattened vectors: -(x - b) / lr of subnormals,
    of values near FLT_MAX (lr = 0.03 overflows them), of NaN and +-inf, by the IEEE division (lr = 98) and
    by the float64 reciprocal product (lr = 0.03); entry borders inside the 64-element chain groups."""
    engine = FedAvgEngine(DEV)
    engine.delta_arenas = deltas
    lay, k = SV.layout(), 5
    for j, (label, case) in enumerate(_arena_cases(lay, k, one_per_client=True)):
        gf, gi = _fedadp_gradient(case, j)
        rnd = _staged_round(engine, case)
        hg = np.zeros(rnd.layout.row_f32, np.float32)
        hg[: lay.n_f32] = gf
        hi = np.zeros(rnd.layout.row_i64, np.float32)
        hi[: lay.n_i64] = gi
        inner, g_sq, l_sq = rnd.fedadp_dots((torch.from_numpy(hg).to(DEV), torch.from_numpy(hi).to(DEV)), range(k), lr)
        w_inner, w_g, w_l = _fedadp_want(case, gf, gi, lr)
        _check(inner, w_inner, f"fedadp inner {label} lr {lr} [client]")
        _check(np.float32(g_sq), w_g, f"fedadp g.g {label} lr {lr}")
        _check(l_sq, w_l, f"fedadp loc.loc {label} lr {lr} [client]")
        engine.release_arrivals()


def _entrywise(engine, case, w, noise, add_base=True):
    lay = case["layout"]
    rnd = _staged_round(engine, case)
    nz = None if noise is None else lay.unpack(torch.from_numpy(noise[0]), torch.from_numpy(noise[1]))
    rnd.launch_entrywise(w, scale=-1.2, noise=nz, noise_scale=0.001, add_base=add_base)
    got = rnd.result()
    return (torch.cat([got[e.name].reshape(-1) for e in lay.entries if e.region == "f32"]).numpy(),
            torch.cat([got[e.name].reshape(-1).float() for e in lay.entries if e.region == "i64"]).numpy())


def _entrywise_weights(case, rng):
    """[n_entries, k] weights: ordinary numbers, 0 and -0 against the special elements (0 x inf = NaN in the
    reference too), and one inf and one NaN weight on ordinary entries."""
    lay, k = case["layout"], case["k"]
    w = rng.standard_normal((len(lay.entries), k))
    names = lay.keys()
    for j, (c, name, _, _) in enumerate(case["targets"]):
        if j % 3 != 2:
            w[names.index(name), c] = 0.0 if j % 3 == 0 else -0.0
    w[names.index("v7"), k - 1] = np.inf
    w[names.index("v129"), 0] = np.nan
    return w


@pytest.mark.parametrize("noise", [False, True], ids=["plain", "noise"])
def test_entrywise_at_special_values(noise):
    """plato_agg_fedavg_entrywise == oracle.entrywise_numpy, one rounding per op: 0 and -0 weights against
    inf, NaN and overflowing deltas, subnormal products, int64 differences of -2^63."""
    engine = FedAvgEngine(DEV)
    lay, k = SV.layout(), 3
    rng = np.random.default_rng(5)
    for label, case in _arena_cases(lay, k, rotations=(0, 2, 4)):
        w = _entrywise_weights(case, rng)
        nz = None
        if noise:
            nz = (rng.standard_normal(lay.n_f32).astype(np.float32), rng.standard_normal(lay.n_i64).astype(np.float32))
        with np.errstate(all="ignore"):
            exp_f, exp_i = FO.entrywise_numpy(lay.entries, case["bf"], case["bi"], list(case["xs_f"]), list(case["xs_i"]),
                                              w, -1.2, None if nz is None else nz[0], None if nz is None else nz[1],
                                              0.001, True)
        got_f, got_i = _entrywise(engine, case, w, nz)
        _check(got_f, exp_f, f"entrywise {label} fp32 region [element]")
        _check(got_i, exp_i, f"entrywise {label} int64 region [element]")


# ------------------------------------------------------------------------------------------------
# containment: one poisoned (client, entry) changes only the outputs that read it
# ------------------------------------------------------------------------------------------------
def _every_output(engine, case, v_f, v_i, grads, w):
    """Each kernel's outputs on a weight-arena case, as {name: array}; float64 ones as uint64-comparable."""
    lay, k = case["layout"], case["k"]
    st = Staged(case, False)
    out = {"entry_norms": _entry_norms(st, lay, k, _norm_tables(lay)),
           "np_sumsq": _np_sumsq(st, k, _sumsq_tables(lay))}
    # Port: every client's delta as one vector
    segs, n_flat = _segments(lay)
    stride = -(-n_flat // 64) * 64
    flat = EC.guarded(k * stride, EC.SENTINEL32, DEV)
    tab = torch.tensor(st.pf + st.pi + [st._bf.data_ptr()] * k + [st._bi.data_ptr()] * k
                       + [flat.data_ptr() + 4 * stride * r for r in range(k)], dtype=torch.int64, device=DEV)
    p, norms = tab.data_ptr(), EC.guarded(k, EC.SENTINEL32, DEV)
    _lib.call("plato_agg_port_norms", p, p + 8 * k, p + 16 * k, p + 24 * k, k, None, segs.data_ptr(), len(lay.entries),
              n_flat, lay.n_f32, 0, norms.data_ptr(), p + 32 * k, _stream())
    out["port_norms"] = _take32(norms, k)
    out["port_flat"] = _take32(flat, k * stride).reshape(k, stride)[:, :n_flat]
    out["client_dots"] = EC.device_dots(dict(k=k, n_f=lay.n_f32, n_i=lay.n_i64, has_base=True, x=case["xs_f"],
                                          xi=case["xs_i"], b=case["bf"], bi=case["bi"], v=v_f[: lay.n_f32],
                                          vi=np.arange(lay.n_i64, dtype=np.int64) - 2), DEV)
    rnd = _staged_round(engine, case)
    dv, dd, vv = rnd.entry_stats(range(k), v=(torch.from_numpy(v_f).to(DEV), torch.from_numpy(v_i).to(DEV)))
    out.update(stats_dv=dv, stats_dd=dd, stats_vv=vv)
    inner, g_sq, l_sq = rnd.fedadp_dots(grads, range(k), 0.03)
    out.update(fedadp_inner=np.asarray(inner), fedadp_g=np.float32(g_sq).reshape(1), fedadp_l=np.asarray(l_sq))
    out["entrywise_f"], out["entrywise_i"] = _entrywise(engine, case, w, None)
    return out


@pytest.fixture(scope="module")
def contained():
    """The clean run, once: ordinary data, checked against the references where the tolerance tests do."""
    engine = FedAvgEngine(DEV)
    lay, k = SV.layout(), 5
    clean = SV.arena_case(lay, k, counters=False)
    rng = np.random.default_rng(9)
    v_f = rng.standard_normal(lay.row_f32).astype(np.float32)
    v_i = rng.standard_normal(lay.row_i64).astype(np.float32)
    g_f = torch.from_numpy((rng.standard_normal(lay.row_f32) * 0.01).astype(np.float32)).to(DEV)
    g_i = torch.from_numpy(rng.standard_normal(lay.row_i64).astype(np.float32)).to(DEV)
    w = rng.standard_normal((len(lay.entries), k))
    extra = (v_f, v_i, (g_f, g_i), w)
    return engine, lay, k, clean, extra, _every_output(engine, clean, *extra)


@pytest.mark.parametrize("client,name,where", [(0, "s0", "first"), (1, "v9", "last"), (4, "v8191", "last"),
                                               (2, "v8192", "first"), (3, "v24579", 8192)])
@pytest.mark.parametrize("kind", ["nan", "inf", "ovf"])
def test_a_poisoned_entry_stays_contained(contained, kind, client, name, where):
    """One (client, entry) holds a NaN, an inf or overflowing values.  Every output that does not read it is
    bit-identical to the clean run (K = 5: np_sumsq's clients share workgroups here; entry_norms runs one
    client per workgroup, its shared and folded kernels have their own containment test above; the two
    float64 kernels are repeatable run to run); the outputs that do read it have the IEEE class and sign of
    the float64 restatements, and where those are finite they keep the tolerance of
    tests/test_per_entry_gpu.py (1e-12 relative)."""
    engine, lay, k, clean, extra, ref_out = contained
    case = SV.poisoned(clean, client, name, kind, where)
    got = _every_output(engine, case, *extra)
    e_i, e = lay.keys().index(name), lay[name]
    piece = [i for i, x in enumerate(lay.entries) if x.region == "f32"].index(e_i)
    el = np.zeros(lay.n_f32, bool)
    el[e.offset:e.offset + e.numel] = True
    hit = {  # the outputs that read (client, entry), as boolean masks
        "entry_norms": (np.arange(k)[:, None] == client) & (np.arange(len(lay.entries))[None, :] == e_i),
        "np_sumsq": (np.arange(k)[:, None] == client) & (np.arange(ref_out["np_sumsq"].shape[1])[None, :] == piece),
        "port_norms": np.arange(k) == client,
        "port_flat": np.broadcast_to((np.arange(k) == client)[:, None], ref_out["port_flat"].shape),
        "client_dots": np.isin(np.arange(2 * k + 1), (client, k + client)),
        "stats_dv": None, "stats_dd": None, "stats_vv": np.zeros(len(lay.entries), bool),
        "fedadp_inner": np.arange(k) == client, "fedadp_g": np.zeros(1, bool), "fedadp_l": np.arange(k) == client,
        "entrywise_f": el, "entrywise_i": np.zeros(lay.n_i64, bool),
    }
    hit["stats_dv"] = hit["stats_dd"] = hit["entry_norms"]
    for key, mask in hit.items():
        a, b = np.ascontiguousarray(got[key]), np.ascontiguousarray(ref_out[key])
        u = np.uint32 if a.dtype == np.float32 else np.uint64
        same = a.view(u) == b.view(u)
        assert same[~mask].all(), (key, "an output that does not read the poisoned entry changed", np.argwhere(~same & ~mask)[:8])
    # the poisoned outputs: class and sign of the float64 restatements
    v_f, v_i = extra[0], extra[1]
    with np.errstate(all="ignore"):
        e_dv, e_dd, _ = FO.entry_stats_fp64(lay.entries, case["bf"], case["bi"], list(case["xs_f"]), list(case["xs_i"]),
                                            v_f, v_i)
        dots_want, dots_bound = EC.dots_reference_general(
            dict(k=k, has_base=True, x=case["xs_f"], xi=case["xs_i"], b=case["bf"], bi=case["bi"], v=v_f[: lay.n_f32],
                 vi=np.arange(lay.n_i64, dtype=np.int64) - 2))
    for key, want in (("stats_dv", e_dv), ("stats_dd", e_dd)):
        g, w_ = got[key][client, e_i], want[client, e_i]
        assert SV.ieee_class(g) == SV.ieee_class(w_), (key, g, w_)
        if np.isfinite(w_):
            np.testing.assert_allclose(g, w_, rtol=1e-12)
    for j in (client, k + client):
        g, w_ = got["client_dots"][j], dots_want[j]
        assert SV.ieee_class(g) == SV.ieee_class(w_), ("client_dots", j, g, w_)
        if np.isfinite(w_):  # the any-order bound of tests/test_client_dots_gpu.py
            assert abs(g - w_) <= dots_bound[j], ("client_dots", j, g, w_, dots_bound[j])
    # the float32 ones: the restatements' bits
    _check(got["entry_norms"][client, e_i], R.torch_norm(SV.entry_rows(case, e)[client]), "poisoned entry_norms")
    with np.errstate(all="ignore"):
        _check(got["np_sumsq"][client, piece], R.np_sum(np.square(SV.entry_rows(case, e)[client])), "poisoned np_sumsq")
        vec = R.port_delta(lay.entries, case["bf"], case["bi"], case["xs_f"][client], case["xs_i"][client])
    _check(got["port_norms"][client], R.torch_norm(vec), "poisoned port_norms")
    _check(got["port_flat"][client], vec, "poisoned port flat row")


def test_clean_run_of_the_containment_tests_matches_the_references(contained):
    """The clean run itself: the float32 outputs bit for bit, the float64 ones within their tolerances."""
    engine, lay, k, clean, (v_f, v_i, grads, w), out = contained
    _check(out["entry_norms"], _want_norms(clean), "entry_norms")
    e_dv, e_dd, e_vv = FO.entry_stats_fp64(lay.entries, clean["bf"], clean["bi"], list(clean["xs_f"]), list(clean["xs_i"]),
                                           v_f, v_i)
    np.testing.assert_allclose(out["stats_dd"], e_dd, rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(out["stats_dv"], e_dv, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(out["stats_vv"], e_vv, rtol=1e-12, atol=1e-300)
    c = dict(k=k, has_base=True, x=clean["xs_f"], xi=clean["xs_i"], b=clean["bf"], bi=clean["bi"], v=v_f[: lay.n_f32],
             vi=np.arange(lay.n_i64, dtype=np.int64) - 2)
    want, bound = EC.dots_reference_general(c)
    assert (np.abs(out["client_dots"] - want) <= bound).all()
    exp_f, exp_i = FO.entrywise_numpy(lay.entries, clean["bf"], clean["bi"], list(clean["xs_f"]), list(clean["xs_i"]), w,
                                      -1.2, None, None, 0.001, True)
    _check(out["entrywise_f"], exp_f, "entrywise fp32")
    _check(out["entrywise_i"], exp_i, "entrywise int64")


# ------------------------------------------------------------------------------------------------
# containment among the clients of one launch: cosine sums, sdot, the folded entry_norms kernels
# ------------------------------------------------------------------------------------------------
def _poison_vector(y: np.ndarray, kind: str, place: int, seed: int) -> np.ndarray:
    """y with a NaN or an inf at `place`, or (ovf) wholly at 1e19..1e20."""
    if kind == "ovf":
        return SV.whole_values("ovf", y.size, np.random.default_rng([13, seed]))
    out = y.copy()
    out[place] = {"nan": np.nan, "inf": np.inf}[kind]
    return out


def _poisonings(n: int, k: int):
    """(victim, kind, place): every client in turn, a NaN and an inf at the first and the last element (the
    tail, where n % 8 != 0), and overflowing values throughout."""
    for j in range(k):
        for kind in ("nan", "inf", "ovf"):
            for place in ((0,) if kind == "ovf" else sorted({0, n - 1})):
                yield j, kind, place


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("n", [9, 1000, 32773])
def test_cosine_sums_contain_a_poisoned_client(n, k):
    """A clean a against K clients of which exactly one holds a NaN, an inf or overflowing values (its
    norm NaN or inf): the other clients' sums are bit-identical to the clean run and to the restatement —
    clients that share a workgroup in pairs or in fours, the odd client whose missing partner recomputes
    client K - 1, one pass and two — through plato_agg_torch_cosine_sum and every scaled variant."""
    rng = np.random.default_rng([n, k])
    a = (rng.standard_normal(n) * 1e-2).astype(np.float32)
    ys = [((rng.standard_normal(n) * 3e-2).astype(np.float32) + a).astype(np.float32) for _ in range(k)]
    n_var = _lib.tune().plato_agg_tune_num_cosine_variants()
    forms = ["plain", None] + list(range(n_var))
    h = _stream()
    na = R.torch_norm(a)
    d_na = torch.from_numpy(np.asarray([na], np.float32)).to(DEV)
    bufa, _ = _rows([a])
    scaled = EC.guarded(n, EC.SENTINEL32, DEV)
    _lib.call("plato_agg_scale_by_norm", bufa.data_ptr(), n, d_na.data_ptr(), EPS, scaled.data_ptr(), h)
    _check(_take32(scaled, n), np.divide(a, na, dtype=np.float32), "scale_by_norm of the clean a")

    def run(vecs, threads):
        bufy, py = _rows(vecs)
        with np.errstate(all="ignore"):
            d_nb = torch.from_numpy(np.asarray([R.torch_norm(y) for y in vecs], np.float32)).to(DEV)
        ws = torch.empty(_lib.lib().plato_agg_torch_cosine_workspace(k, threads) // 4 + 1, device=DEV)
        outs = {}
        for f in forms:
            out = EC.guarded(k, EC.SENTINEL32, DEV)
            if f == "plain":
                _lib.call("plato_agg_torch_cosine_sum", bufa.data_ptr(), py.data_ptr(), k, n, d_na.data_ptr(),
                          d_nb.data_ptr(), EPS, threads, ws.data_ptr(), out.data_ptr(), h)
            else:
                args = (scaled.data_ptr(), py.data_ptr(), k, n, d_nb.data_ptr(), EPS, threads, ws.data_ptr(),
                        out.data_ptr(), h)
                if f is None:
                    _lib.call("plato_agg_torch_cosine_sum_scaled", *args)
                else:
                    _lib.tune_call("plato_agg_tune_torch_cosine_sum_scaled", f, *args)
            outs[f] = _take32(out, k)
        return outs

    for threads in (1, 4):
        clean = run(ys, threads)
        want_clean = np.asarray([R.torch_cosine(a, y, threads) for y in ys])
        for f in forms:
            _check(clean[f], want_clean, f"clean cosine sums, form {f}, threads {threads}")
        for j, kind, place in _poisonings(n, k):
            vecs = list(ys)
            vecs[j] = _poison_vector(ys[j], kind, place, j)
            with np.errstate(all="ignore"):
                want_j = R.torch_cosine(a, vecs[j], threads)
            assert kind == "ovf" or np.isnan(want_j), (kind, want_j)  # ovf: the norm is inf, every quotient 0
            got = run(vecs, threads)
            others = np.arange(k) != j
            for f in forms:
                what = f"cosine form {f}, n {n}, K {k}, threads {threads}, client {j} holds {kind} at {place}"
                assert got[f][others].tobytes() == clean[f][others].tobytes(), what + ": another client's sum changed"
                _check(got[f][j], want_j, what + ": the poisoned client's own sum")


@pytest.mark.parametrize("npairs", [3, 9])
@pytest.mark.parametrize("n", [33, 64, 4097])
def test_sdot_contains_a_poisoned_pair(n, npairs):
    """A clean x against n_pairs y rows of which exactly one holds a NaN, an inf or overflowing values: the
    other pairs' x.y and y.y are bit-identical to the clean run and to the restatement, in
    plato_agg_sdot_pairs and in every plato_agg_sdot_shared variant (pairs that share a workgroup's read of
    x), with and without x.x."""
    rng = np.random.default_rng([n, npairs, 1])
    x = rng.standard_normal(n).astype(np.float32)
    ys = [(rng.standard_normal(n) * 1e-2).astype(np.float32) for _ in range(npairs)]
    n_var = _lib.tune().plato_agg_tune_num_sdot_shared_variants()
    forms = ["pairs"] + [(v, xx) for v in [None] + list(range(n_var)) for xx in (0, 1)]
    ws = torch.empty(_lib.lib().plato_agg_sdot_shared_workspace(npairs, 1) // 4, dtype=torch.float32, device=DEV)
    bx, px = _rows([x] * npairs)
    h = _stream()

    def run(vecs):
        by, py = _rows(vecs)
        outs = {}
        for f in forms:
            m = npairs + (0 if f == "pairs" else f[1])
            o_xy, o_yy = EC.guarded(m, EC.SENTINEL32, DEV), EC.guarded(m, EC.SENTINEL32, DEV)
            if f == "pairs":
                _lib.call("plato_agg_sdot_pairs", px.data_ptr(), py.data_ptr(), npairs, n, o_xy.data_ptr(),
                          o_yy.data_ptr(), h)
            else:
                args = (bx.data_ptr(), py.data_ptr(), npairs, n, f[1], ws.data_ptr(), o_xy.data_ptr(), o_yy.data_ptr(), h)
                if f[0] is None:
                    _lib.call("plato_agg_sdot_shared", *args)
                else:
                    _lib.tune_call("plato_agg_tune_sdot_shared", f[0], *args)
            outs[f] = np.stack([_take32(o_xy, m), _take32(o_yy, m)])
        return outs

    def want(vecs, m):
        with np.errstate(all="ignore"):
            xx = R.sdot(x, x)
            return np.asarray([[R.sdot(x, y) for y in vecs] + [xx], [R.sdot(y, y) for y in vecs] + [xx]])[:, :m]

    clean = run(ys)
    for f in forms:
        _check(clean[f], want(ys, clean[f].shape[1]), f"clean sdot, form {f}")
    for j, kind, place in _poisonings(n, npairs):
        vecs = list(ys)
        vecs[j] = _poison_vector(ys[j], kind, place, j)
        got = run(vecs)
        for f in forms:
            what = f"sdot form {f}, n {n}, pair {j} of {npairs} holds {kind} at {place}"
            others = np.arange(got[f].shape[1]) != j
            assert got[f][:, others].tobytes() == clean[f][:, others].tobytes(), what + ": another pair's dots changed"
            w = want(vecs, got[f].shape[1])
            assert not np.isfinite(w[1, j]), (kind, w[:, j])
            _check(got[f][:, j], w[:, j], what + ": the poisoned pair's own dots")


NORMS_SHARING_VARIANTS = tuple(range(9, 17))  # two and four clients per workgroup: two chain waves, or folded into one


@pytest.mark.parametrize("deltas", [False, True], ids=["weight_arenas", "delta_arenas"])
@pytest.mark.parametrize("k", [97, 128])
def test_entry_norms_sharing_a_workgroup_contain_a_poisoned_client(k, deltas):
    """The kernels in which the clients of one entry share a workgroup, its baseline tiles and (folded) one
    chain wave — the default from K = 96 (two clients, K = 97: a ragged last group that recomputes client
    K - 1) and from K = 128 (four), and tuning variants 9-16 — on the whole layout, so that they walk tile
    borders: with one (client, entry) poisoned, every other norm is bit-identical to the clean run, the
    poisoned one the restatement's."""
    lay = SV.layout()
    tabs = _norm_tables(lay)
    assert _lib.tune().plato_agg_tune_num_entry_norms_variants() > max(NORMS_SHARING_VARIANTS)
    variants = [None] + list(NORMS_SHARING_VARIANTS)
    clean_case = SV.arena_case(lay, k)
    st = Staged(clean_case, deltas)
    clean = {v: _entry_norms(st, lay, k, tabs, v) for v in variants}
    want_clean = _want_norms(clean_case)
    for v in variants:
        _check(clean[v], want_clean, f"clean entry_norms, K {k}, variant {v}")
    names = lay.keys()
    # a client in the middle of a group of two and of four, the last of a group, the last client (K = 97: alone in
    # its group), against entries that are scalar, end or begin next to a tile-long neighbour, or span tiles
    for client, name, where, kind in [(5, "s0", "first", "inf"), (6, "v8191", "last", "nan"), (k - 1, "v8192", "first", "ovf"),
                                      (k - 2, "v24579", 8192, "inf"), (0, "v24579", "last", "nan"), (k - 1, "v9", "last", "inf")]:
        case = SV.poisoned(clean_case, client, name, kind, where)
        rows = (SV.arena_deltas(case)[0] if deltas else case["xs_f"])[client]
        keep = st.xf[client, : lay.n_f32].clone()
        st.xf[client, : lay.n_f32] = torch.from_numpy(np.ascontiguousarray(rows)).to(DEV)
        e_i = names.index(name)
        with np.errstate(all="ignore"):
            want = R.torch_norm(SV.entry_rows(case, lay[name])[client])
        mask = np.ones(clean[None].shape, bool)
        mask[client, e_i] = False
        for v in variants:
            got = _entry_norms(st, lay, k, tabs, v)
            what = f"entry_norms K {k} variant {v}: client {client}'s {name} holds {kind}"
            assert got[mask].tobytes() == clean[v][mask].tobytes(), what + ": another norm changed"
            _check(got[client, e_i], want, what + ": the poisoned norm")
        st.xf[client, : lay.n_f32] = keep
