"""The robust aggregators' pieces at K x ResNet-18, HIP events, interleaved in one process.

    python scripts/bench_robust.py --algo krum|bulyan|fltrust [--ks 128,256] [--reps 10] [--host-ks 16,32]
    python scripts/bench_robust.py --algo lie|minmax|minsum [--ks 20,32] [--reps 10] [--host-ks 4,8]

Per K the algorithm's kernels and the fused FedAvg kernel on the same rows (the streaming yardstick) run in
turn in every repetition; median and minimum over the repetitions.

krum: plato_agg_pairwise_sqdist, plato_agg_mean_rows over the K - 6 selected rows, and the host selection
(plato_amd.krum) on the device's matrix; the distance kernel's floors from the MI355X's vector rate and HBM
bandwidth beside it.  --host-ks: one selection step's distance loop of the reference
(`torch.norm(X - X[i], dim=1) ** 2` for each i, aggregations.py:186-192).

bulyan: the median kernel (plato_agg_robust_columns, mode 0), the nearest-mean kernel (mode 1) over all K
rows with trim 0 and trim 3, Bulyan's three stages with f = 3 (plato_agg_pairwise_sqdist, the host selection
of plato_amd.krum.bulyan_select, the nearest-mean kernel over the theta selected rows with trim 3); every
nearest-mean time as a ratio to the median kernel's of the same run.  --host-ks: aggregations.py:238-243
(`median`, `argsort(abs(X - med))`, the gather, `mean`).

fltrust: plato_agg_mean_rows over the K rows, plato_agg_trust_stats against that mean, plato_agg_scaled_sum
with the scalars the statistics give (plato_amd.trust); the achieved GB/s of each (K rows read and one fp32
row besides: the result written, or the mean read), its ratio to mean_rows, and the HBM floor of one pass.
--host-ks: aggregations.py:408-441 (torch.mean, the dot / norm loop, the clip, the candidates built by
torch.cat and their torch.sum) from the flattened matrix on (flatten_weights, quadratic in copies, is not
timed).

lie, minmax, minsum (K is the number of attackers A): the attackers' delta rows are formed
once (plato_agg_compute_deltas, timed apart).  lie: plato_agg_column_std beside plato_agg_mean_rows over the
same delta rows (the two stream the same bytes) and plato_agg_add_scaled_rows into the weight rows; GB/s of
each and column_std's ratio to mean_rows and to the HBM read rate.  minmax / minsum: the kernels of the
search attacks (mean_rows, trust_stats against the average and against the unit vector, scale_by_norm,
pairwise_sqdist, add_scaled_rows) and the host search (plato_amd.attacks) on the device's statistics.
--host-ks: the attack's op sequence after flatten_weights (attacks.py:186-199 for lie; :247-287 and
:379-419 for the searches: the A x A distance loop and the search's passes of `torch.norm(X - v, dim=1) ** 2`).

--host-ks runs the reference's own op sequence on this host's CPU at 16 threads, on the same synthetic rows.
"""

from __future__ import annotations

import argparse
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from plato_amd import _lib, attacks, workloads  # noqa: E402
from plato_amd.arena import ArenaLayout  # noqa: E402
from plato_amd.engine import ClientSlab, DeviceArena, FedAvgEngine, fedavg_weights, fp32_weights  # noqa: E402
from plato_amd.krum import bulyan_select, multi_krum_select  # noqa: E402
from plato_amd.synthetic import fill_baseline, fill_clients  # noqa: E402
from plato_amd.trust import EPS, fltrust_weights  # noqa: E402

# MI355X: 256 CUs x 4 SIMDs x 32 lanes per clock at 2.4 GHz; HBM3E as measured by a float4 copy
LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9
HBM_BYTES_PER_S = 6.29e12
TILE = 32
F = 3  # bulyan
MEDIAN, NEAREST = _lib.PLATO_AGG_ROBUST["median"], _lib.PLATO_AGG_ROBUST["nearest_mean"]


def host_ms(fn, reps: int = 5):
    """(fn's last result, its host times in ms)"""
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        got = fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return got, times


def tables(b, rows):
    pf, pi = b.slab.row_pointers(rows)
    return torch.from_numpy(pf).to(b.dev), torch.from_numpy(pi).to(b.dev)


def outputs(b):
    """The result rows and FedAvg's weights, allocated after the algorithm's own buffers: the order of the
    scripts that recorded profiles/r08a_krum.log, r09a_bulyan.log and r10a_fltrust.log."""
    b.out_f = torch.empty(b.layout.row_f32, dtype=torch.float32, device=b.dev)
    b.out_i = torch.empty(b.layout.row_i64, dtype=torch.float32, device=b.dev)
    b.w = torch.from_numpy(fp32_weights(fedavg_weights([1000] * b.k))).to(b.dev)


def sqdist_and_selection(b, select):
    """(the distance kernel, its workspace, the rows `select` picks from the device's matrix, select's times)"""
    work = torch.empty(_lib.lib().plato_agg_pairwise_sqdist_workspace(b.k, b.n_f, b.n_i), dtype=torch.uint8, device=b.dev)
    dist = torch.empty((b.k, b.k), dtype=torch.float64, device=b.dev)
    outputs(b)

    def sqdist():
        _lib.call("plato_agg_pairwise_sqdist", b.tf.data_ptr(), b.ti.data_ptr(), b.k, b.n_f, b.n_i, work.data_ptr(),
                  dist.data_ptr(), b.sh)

    sqdist()
    torch.cuda.synchronize()
    host = dist.cpu().numpy()
    sel, select_ms = host_ms(lambda: select(host))
    return sqdist, work, sel, select_ms


# ---------------------------------------------------------------------- per algorithm: kernels and report
def krum_device(b):
    k, n_f, n_i = b.k, b.n_f, b.n_i
    sqdist, work, sel, select_ms = sqdist_and_selection(b, lambda host: multi_krum_select(host, 2))
    sf, si = tables(b, sel)

    def mean():
        _lib.call("plato_agg_mean_rows", sf.data_ptr(), si.data_ptr(), len(sel), b.out_f.data_ptr(), b.out_i.data_ptr(),
                  n_f, n_i, b.sh)

    def report(times):
        d = n_f + n_i
        pairs = k * (k - 1) // 2
        valu_ms = pairs * d * 2 / LANE_OPS_PER_S * 1e3           # one v_sub_f32 and one v_fma_f32 per pair and coordinate
        hbm_ms = k * d * 4 / HBM_BYTES_PER_S * 1e3                # every row once
        t = -(-k // TILE)
        tiled_gb = t * (t + 1) // 2 * 2 * TILE * d * 4 / 1e9      # 64 rows per 32 x 32 tile (mostly L2 / Infinity Cache hits)
        print(f"K={k} D={d} reps={b.reps} selected={len(sel)} workspace_MB={work.numel() / 1e6:.1f}")
        for name, ms in times.items():
            line = f"  {name:16s} median {statistics.median(ms):9.3f} ms   min {min(ms):9.3f} ms"
            if name == "pairwise_sqdist":
                line += (f"   VALU floor {valu_ms:.3f} ms ({valu_ms / statistics.median(ms):.1%} of the median; binds)"
                         f"   HBM floor {hbm_ms:.3f} ms   tiled reads {tiled_gb:.1f} GB")
            else:
                rows = len(sel) if name == "mean_rows" else k + 1
                gb = (rows * (n_f * 4 + n_i * 8) + (n_f + n_i) * 4) / 1e9
                line += f"   {gb / statistics.median(ms) * 1e3:8.1f} GB/s"
            print(line)
        print(f"  host selection   median {statistics.median(select_ms):9.3f} ms   min {min(select_ms):9.3f} ms")

    return {"pairwise_sqdist": sqdist, "mean_rows": mean}, report


def bulyan_device(b):
    k, n_f, n_i = b.k, b.n_f, b.n_i
    sqdist, _, sel, select_ms = sqdist_and_selection(b, lambda host: bulyan_select(host, F))
    sf, si = tables(b, sel)

    def columns(mode, trim, rows_f=b.tf, rows_i=b.ti, rows=k):
        return lambda: _lib.call("plato_agg_robust_columns", mode, rows_f.data_ptr(), rows_i.data_ptr(), rows, trim,
                                 b.out_f.data_ptr(), b.out_i.data_ptr(), n_f, n_i, b.sh)

    def report(times):
        print(f"K={k} D={n_f + n_i} reps={b.reps} f={F} theta={len(sel)}")
        med = {name: statistics.median(ms) for name, ms in times.items()}
        for name, ms in times.items():
            rows = len(sel) if "theta" in name else k + (name == "fedavg")
            gb = (rows * (n_f * 4 + n_i * 8) + (n_f + n_i) * 4) / 1e9  # every row once, the result once
            line = f"  {name:34s} median {med[name]:9.3f} ms   min {min(ms):9.3f} ms"
            if "sqdist" not in name:
                line += f"   {gb / med[name] * 1e3:8.1f} GB/s"
            if "nearest_mean" in name:
                line += f"   {med[name] / med['robust_median']:.2f} x robust_median"
            print(line)
        print(f"  {'bulyan: host selection':34s} median {statistics.median(select_ms):9.3f} ms   min {min(select_ms):9.3f} ms")

    return {"robust_median": columns(MEDIAN, 0), "nearest_mean trim 0": columns(NEAREST, 0),
            f"nearest_mean trim {F}": columns(NEAREST, F), "bulyan: pairwise_sqdist": sqdist,
            f"bulyan: nearest_mean theta={len(sel)}": columns(NEAREST, F, sf, si, len(sel))}, report


def fltrust_device(b):
    k, n_f, n_i = b.k, b.n_f, b.n_i
    work = torch.empty(_lib.lib().plato_agg_trust_stats_workspace(k, n_f, n_i), dtype=torch.uint8, device=b.dev)
    stats = torch.empty(3 * k + 1, dtype=torch.float64, device=b.dev)
    mean_f = torch.empty(b.layout.row_f32, dtype=torch.float32, device=b.dev)
    mean_i = torch.empty(b.layout.row_i64, dtype=torch.float32, device=b.dev)
    outputs(b)

    def mean():
        _lib.call("plato_agg_mean_rows", b.tf.data_ptr(), b.ti.data_ptr(), k, mean_f.data_ptr(), mean_i.data_ptr(),
                  n_f, n_i, b.sh)

    def trust_stats():
        _lib.call("plato_agg_trust_stats", b.tf.data_ptr(), b.ti.data_ptr(), k, mean_f.data_ptr(), mean_i.data_ptr(), EPS,
                  n_f, n_i, work.data_ptr(), stats.data_ptr(), b.sh)

    mean()
    trust_stats()
    torch.cuda.synchronize()
    host_stats = stats.cpu().numpy()
    scal, scalar_ms = host_ms(lambda: fltrust_weights(host_stats, k, EPS))
    table = torch.from_numpy(np.concatenate([scal["weights"], scal["div"]])).to(b.dev)

    def scaled_sum():
        _lib.call("plato_agg_scaled_sum", b.tf.data_ptr(), b.ti.data_ptr(), k, table.data_ptr(), table.data_ptr() + 4 * k,
                  float(scal["nm"]), b.out_f.data_ptr(), b.out_i.data_ptr(), n_f, n_i, b.sh)

    def report(times):
        d = n_f + n_i
        row_bytes = n_f * 4 + n_i * 8
        floor_ms = k * row_bytes / HBM_BYTES_PER_S * 1e3
        print(f"K={k} D={d} reps={b.reps} workspace_MB={work.numel() / 1e6:.1f} clipped={int((scal['cos'] < 0).sum())} "
              f"HBM floor of one pass {floor_ms:.3f} ms")
        medians = {name: statistics.median(ms) for name, ms in times.items()}
        for name, ms in times.items():
            rows = k + 1 if name == "fedavg" else k
            gb = (rows * row_bytes + d * 4) / 1e9  # one fp32 row besides: the result written, or the mean read
            print(f"  {name:12s} median {medians[name]:9.3f} ms   min {min(ms):9.3f} ms   max {max(ms):9.3f} ms"
                  f"   {gb / medians[name] * 1e3:8.1f} GB/s   {medians[name] / medians['mean_rows']:.2f} x mean_rows")
        total = medians["mean_rows"] + medians["trust_stats"] + medians["scaled_sum"]
        print(f"  Fl-trust kernels (mean_rows + trust_stats + scaled_sum) {total:9.3f} ms; host scalars "
              f"median {statistics.median(scalar_ms):.3f} ms")

    return {"mean_rows": mean, "trust_stats": trust_stats, "scaled_sum": scaled_sum}, report


def attack_device(kind):
    def device(b):
        a, n_f, n_i, lay = b.k, b.n_f, b.n_i, b.layout
        df = torch.empty((a, lay.row_f32), dtype=torch.float32, device=b.dev)
        di = torch.empty((a, lay.row_i64), dtype=torch.int64, device=b.dev)
        dtf = torch.tensor([df[j].data_ptr() for j in range(a)], dtype=torch.int64, device=b.dev)
        dti = torch.tensor([di[j].data_ptr() for j in range(a)], dtype=torch.int64, device=b.dev)
        row = lambda: (torch.empty(lay.row_f32, dtype=torch.float32, device=b.dev),  # noqa: E731
                       torch.empty(lay.row_i64, dtype=torch.float32, device=b.dev))
        (avg_f, avg_i), (v_f, v_i) = row(), row()
        pf, pi = b.slab.row_pointers(range(a))

        def deltas():
            for j in range(a):
                _lib.call("plato_agg_compute_deltas", int(pf[j]), int(pi[j]), b.base.f32.data_ptr(), b.base.i64.data_ptr(),
                          df[j].data_ptr(), di[j].data_ptr(), n_f, n_i, b.sh)

        def mean(tf=dtf, ti=dti):
            _lib.call("plato_agg_mean_rows", tf.data_ptr(), ti.data_ptr(), a, avg_f.data_ptr(), avg_i.data_ptr(), n_f, n_i, b.sh)

        def std():
            _lib.call("plato_agg_column_std", dtf.data_ptr(), dti.data_ptr(), a, v_f.data_ptr(), v_i.data_ptr(), n_f, n_i, b.sh)

        def add(s):
            return lambda: _lib.call("plato_agg_add_scaled_rows", b.tf.data_ptr(), b.ti.data_ptr(), a, s, v_f.data_ptr(),
                                     v_i.data_ptr(), n_f, n_i, b.sh)

        deltas()
        outputs(b)
        row_bytes = n_f * 4 + n_i * 8
        d = n_f + n_i

        def lines(times, gb_of):
            med = {name: statistics.median(ms) for name, ms in times.items()}
            for name, ms in times.items():
                line = f"  {name:18s} median {med[name]:9.3f} ms   min {min(ms):9.3f} ms   max {max(ms):9.3f} ms"
                if name in gb_of:
                    line += f"   {gb_of[name] / med[name] * 1e3:8.1f} GB/s   {med[name] / med['mean_rows']:.2f} x mean_rows"
                print(line)
            return med

        if kind == "lie":
            s = -float(np.float32(attacks.lie_z(100, a)))

            def report(times):
                read = (a * row_bytes + d * 4) / 1e9  # A rows read, one fp32 row written
                print(f"A={a} D={d} reps={b.reps} HBM floor of one read pass {a * row_bytes / HBM_BYTES_PER_S * 1e3:.3f} ms")
                med = lines(times, {"mean_rows": read, "column_std": read, "fedavg": read + row_bytes / 1e9,
                                    "add_scaled_rows": (2 * a * row_bytes + d * 4) / 1e9,
                                    "compute_deltas": 3 * a * row_bytes / 1e9})
                print(f"  column_std reads at {read / med['column_std'] * 1e3 / (HBM_BYTES_PER_S / 1e9):.1%} of the HBM read rate; "
                      f"LIE kernels (compute_deltas + column_std + add_scaled_rows) "
                      f"{med['compute_deltas'] + med['column_std'] + med['add_scaled_rows']:.3f} ms")

            return {"mean_rows": mean, "column_std": std, "add_scaled_rows": add(s), "compute_deltas": deltas}, report

        minsum = kind == "minsum"
        stats_work = torch.empty(_lib.lib().plato_agg_trust_stats_workspace(a, n_f, n_i), dtype=torch.uint8, device=b.dev)
        s_avg = torch.zeros(3 * a + 1, dtype=torch.float64, device=b.dev)
        s_p = torch.zeros(3 * a + 1, dtype=torch.float64, device=b.dev)
        s_ap = torch.zeros(8, dtype=torch.float64, device=b.dev)
        atab = torch.tensor([avg_f.data_ptr(), avg_i.data_ptr()], dtype=torch.int64, device=b.dev)
        d_norm = torch.zeros(1, dtype=torch.float32, device=b.dev)
        dist_work = torch.empty(_lib.lib().plato_agg_pairwise_sqdist_workspace(a, n_f, n_i), dtype=torch.uint8, device=b.dev)
        dist = torch.empty((a, a), dtype=torch.float64, device=b.dev)
        the_mean = (lambda: mean(b.tf, b.ti)) if minsum else mean  # Min-Sum: the mean of the weights

        def stats(ref_f, ref_i, out):
            return lambda: _lib.call("plato_agg_trust_stats", dtf.data_ptr(), dti.data_ptr(), a, ref_f.data_ptr(),
                                     ref_i.data_ptr(), 0.0, n_f, n_i, stats_work.data_ptr(), out.data_ptr(), b.sh)

        def unit():
            _lib.call("plato_agg_scale_by_norm", avg_f.data_ptr(), n_f, d_norm.data_ptr(), 0.0, v_f.data_ptr(), b.sh)
            _lib.call("plato_agg_scale_by_norm", avg_i.data_ptr(), n_i, d_norm.data_ptr(), 0.0, v_i.data_ptr(), b.sh)

        def avg_dot_unit():
            _lib.call("plato_agg_trust_stats", atab.data_ptr(), None, 1, v_f.data_ptr(), None, 0.0, n_f, 0,
                      stats_work.data_ptr(), s_ap.data_ptr(), b.sh)
            _lib.call("plato_agg_trust_stats", atab.data_ptr() + 8, None, 1, v_i.data_ptr(), None, 0.0, n_i, 0,
                      stats_work.data_ptr(), s_ap.data_ptr() + 32, b.sh)

        def sqdist():
            _lib.call("plato_agg_pairwise_sqdist", dtf.data_ptr(), dti.data_ptr(), a, n_f, n_i, dist_work.data_ptr(),
                      dist.data_ptr(), b.sh)

        the_mean()
        stats(avg_f, avg_i, s_avg)()
        torch.cuda.synchronize()
        h_avg = s_avg.cpu().numpy()
        d_norm.copy_(torch.from_numpy(np.asarray([np.sqrt(h_avg[3 * a])], dtype=np.float32)))
        unit()
        stats(v_f, v_i, s_p)()
        avg_dot_unit()
        sqdist()
        torch.cuda.synchronize()
        h_p, h_ap, h_dist = s_p.cpu().numpy(), s_ap.cpu().numpy(), dist.cpu().numpy()
        st = attacks.SearchStats(uu=h_avg[a:2 * a], ua=h_avg[:a], up=h_p[:a], aa=float(h_avg[3 * a]), pp=float(h_p[3 * a]),
                                 ap=float(h_ap[0] + h_ap[4]))
        search = attacks.min_sum_lambda if minsum else attacks.min_max_lambda
        lam, search_ms = host_ms(lambda: search(st, h_dist))

        def report(times):
            read = (a * row_bytes + d * 4) / 1e9
            print(f"A={a} D={d} reps={b.reps} lambda={float(lam)!r} HBM floor of one read pass "
                  f"{a * row_bytes / HBM_BYTES_PER_S * 1e3:.3f} ms")
            med = lines(times, {"mean_rows": read, "stats vs avg": read, "stats vs unit": read,
                                "add_scaled_rows": (2 * a * row_bytes + d * 4) / 1e9, "compute_deltas": 3 * a * row_bytes / 1e9})
            kernels = sum(v for name, v in med.items() if name != "fedavg")
            print(f"  host search        median {statistics.median(search_ms):9.3f} ms   min {min(search_ms):9.3f} ms")
            print(f"  {kind} kernels {kernels:.3f} ms + host search {statistics.median(search_ms):.3f} ms")

        return {"mean_rows": the_mean, "stats vs avg": stats(avg_f, avg_i, s_avg), "unit vector": unit,
                "stats vs unit": stats(v_f, v_i, s_p), "avg . unit": avg_dot_unit, "pairwise_sqdist": sqdist,
                "add_scaled_rows": add(float(lam) if minsum else -float(lam)), "compute_deltas": deltas}, report

    return device


# ---------------------------------------------------------------------- per algorithm: the reference on the host
def krum_host(x, k, n):
    """One selection step's distance loop of the reference."""
    def step():
        for weight in x:
            torch.norm((x - weight), dim=1) ** 2

    yield "one step's distance loop", step


def bulyan_host(x, k, n):
    """aggregations.trimmed_mean's op sequence after flatten_weights."""
    def ops(trim):
        med = torch.median(x, dim=0)[0]
        idx = torch.argsort(torch.abs(x - med), dim=0)
        srt = x[idx, torch.arange(n)[None, :]]
        torch.mean(srt[: k - 2 * trim], dim=0)

    for trim in (0, F):
        yield "median, argsort, gather, mean", lambda trim=trim: ops(trim), f" trim={trim}"


def fltrust_host(flattened_weights, k, n):
    """aggregations.fl_trust from the flattened matrix on."""
    def ops():
        model_re = torch.mean(flattened_weights, dim=0).squeeze()
        cos_sims, candidates = [], []
        for weight in flattened_weights:
            cos_sim = (torch.dot(weight.squeeze(), model_re) / (torch.norm(model_re) + 1e-9)
                       / (torch.norm(weight.squeeze()) + 1e-9))
            cos_sims = cos_sim.unsqueeze(0) if not len(cos_sims) else torch.cat((cos_sims, cos_sim.unsqueeze(0)))
        cos_sims = torch.maximum(cos_sims, torch.tensor(0))
        normalized_weights = cos_sims / (torch.sum(cos_sims) + 1e-9)
        for i in range(k):
            candidate = (flattened_weights[i] * normalized_weights[i] / torch.norm(flattened_weights[i] + 1e-9)
                         * torch.norm(model_re))
            candidates = candidate.unsqueeze(0) if not len(candidates) else torch.cat((candidates, candidate.unsqueeze(0)))
        torch.sum(candidates, dim=0)

    yield "fl_trust after flatten_weights", ops


def lie_host(x, k, n):
    """lie_attack after flatten_weights: the mean it forms and does not use, the std, the product."""
    def ops():
        torch.mean(x, dim=0)
        0.7549 * (-1 * torch.std(x, dim=0))

    yield "mean, std, scale", ops


def search_host(keep_failed):
    """min_max_attack / min_sum_attack after flatten_weights: the A x A distance loop and the search, each
    step one pass of `torch.norm(X - v, dim=1) ** 2`."""
    def host(x, k, n):
        def ops():
            avg = torch.mean(x, 0)
            p = avg / torch.norm(avg)
            limit = torch.tensor([0.0])
            for row in x:
                dist = torch.norm((x - row), dim=1) ** 2
                limit = torch.min(limit, torch.sum(dist)) if keep_failed else torch.max(limit, torch.max(dist))

            def meets(lam):
                dist = torch.norm((x - (avg - float(lam) * p)), dim=1) ** 2
                return bool((torch.sum(dist) if keep_failed else torch.max(dist)) <= limit)

            attacks.halving_search(meets, keep_failed)

        yield "distance loop and search", ops

    return host


ALGOS = {"krum": (krum_device, krum_host), "bulyan": (bulyan_device, bulyan_host),
         "fltrust": (fltrust_device, fltrust_host), "lie": (attack_device("lie"), lie_host),
         "minmax": (attack_device("minmax"), search_host(False)), "minsum": (attack_device("minsum"), search_host(True))}
ATTACKS = ("lie", "minmax", "minsum")


# ---------------------------------------------------------------------- shared
def device_part(algo, k: int, reps: int, layout, dev):
    engine = FedAvgEngine(dev)
    base, slab = DeviceArena(layout, dev), ClientSlab(layout, k, dev)
    fill_baseline(base, 23)
    fill_clients(slab, base, 23, k)
    stream = torch.cuda.current_stream(dev)
    b = SimpleNamespace(k=k, reps=reps, dev=dev, layout=layout, slab=slab, base=base, n_f=layout.n_f32,
                        n_i=layout.n_i64, sh=stream.cuda_stream)
    b.tf, b.ti = tables(b, range(k))
    kernels, report = algo(b)

    def fedavg():
        engine.launch_fedavg(layout, b.tf, b.ti, b.w, None, k, base.f32, base.i64, b.out_f, b.out_i, stream)

    kernels["fedavg"] = fedavg
    for fn in kernels.values():  # warm-up of every shape
        fn()
    torch.cuda.synchronize()
    events = {name: [] for name in kernels}
    for _ in range(reps):
        for name, fn in kernels.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            events[name].append((e0, e1))
    torch.cuda.synchronize()
    report({name: [e0.elapsed_time(e1) for e0, e1 in evs] for name, evs in events.items()})
    sys.stdout.flush()
    del slab, base, b, kernels, report
    torch.cuda.empty_cache()


def host_part(algo, k: int, layout):
    from oracle import synth

    n = layout.n_f32 + layout.n_i64
    bf, bi = synth.baseline_arena(layout.n_f32, layout.n_i64, 23)
    rows = []
    for c in range(k):
        xf, xi = synth.client_arena(bf, bi, 23, c)
        rows.append(torch.cat((torch.from_numpy(xf), torch.from_numpy(xi))))  # promotes the counters, as flatten_weights
    x = torch.stack(rows)
    assert x.shape == (k, n) and x.dtype == torch.float32
    for what, ops, *case in algo(x, k, n):
        _, times = host_ms(ops, 3)
        print(f"host K={k} D={n}{''.join(case)} threads={torch.get_num_threads()}: {what} "
              f"median {statistics.median(times):.1f} ms  min {min(times):.1f} ms")
        sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--algo", required=True, choices=sorted(ALGOS))
    ap.add_argument("--ks", default=None, help="default: 128,256 (the attacks: 20,32 attackers)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-ks", default=None, help="default: 16,32 (the attacks: 4,8)")
    args = ap.parse_args()
    attack = args.algo in ATTACKS
    args.ks = args.ks if args.ks is not None else ("20,32" if attack else "128,256")
    args.host_ks = args.host_ks if args.host_ks is not None else ("4,8" if attack else "16,32")
    on_device, on_host = ALGOS[args.algo]
    layout = ArenaLayout.from_shapes(workloads.resnet(18, 10))
    if args.ks:
        if not torch.cuda.is_available():
            raise SystemExit(f"bench_robust --algo {args.algo}: no GPU (the device part measures nothing without one)")
        dev = torch.device("cuda:0")
        print(torch.cuda.get_device_name(0))
        for k in (int(v) for v in args.ks.split(",")):
            device_part(on_device, k, args.reps, layout, dev)
    if args.host_ks:
        torch.set_num_threads(16)
        for k in (int(v) for v in args.host_ks.split(",")):
            host_part(on_host, k, layout)


if __name__ == "__main__":
    main()
