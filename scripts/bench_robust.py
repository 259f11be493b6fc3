"""The robust aggregators' pieces at K x ResNet-18, HIP events, interleaved in one process.

    python scripts/bench_robust.py --algo krum|bulyan|fltrust [--ks 128,256] [--reps 10] [--host-ks 16,32]

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

from plato_amd import _lib, workloads  # noqa: E402
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


ALGOS = {"krum": (krum_device, krum_host), "bulyan": (bulyan_device, bulyan_host),
         "fltrust": (fltrust_device, fltrust_host)}


# ---------------------------------------------------------------------- shared
def device_part(algo, k: int, reps: int, layout, dev):
    engine = FedAvgEngine(dev)
    base, slab = DeviceArena(layout, dev), ClientSlab(layout, k, dev)
    fill_baseline(base, 23)
    fill_clients(slab, base, 23, k)
    stream = torch.cuda.current_stream(dev)
    b = SimpleNamespace(k=k, reps=reps, dev=dev, layout=layout, slab=slab, n_f=layout.n_f32, n_i=layout.n_i64,
                        sh=stream.cuda_stream)
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
    ap.add_argument("--ks", default="128,256")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-ks", default="16,32")
    args = ap.parse_args()
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
