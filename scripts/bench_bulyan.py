"""Bulyan's and Trimmed-mean's pieces at K x ResNet-18, HIP events, interleaved in one process.

    python scripts/bench_bulyan.py [--ks 128,256] [--reps 10] [--host-ks 16,32]

Per K: the median kernel (plato_agg_robust_columns, mode 0), the nearest-mean kernel (mode 1) over all K
rows with trim 0 and trim 3, Bulyan's three stages with f = 3 (plato_agg_pairwise_sqdist, the host
selection of plato_amd.krum.bulyan_select, the nearest-mean kernel over the theta selected rows with
trim 3), and the fused FedAvg kernel on the same rows (the streaming yardstick).  Each repetition runs
the kernels in turn; median and minimum over the repetitions, and every nearest-mean time as a ratio to
the median kernel's of the same run.

--host-ks: the reference's own op sequence on this host's CPU at 16 threads (aggregations.py:238-243:
`median`, `argsort(abs(X - med))`, the gather, `mean`) on the same synthetic rows.
"""

from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from plato_amd import _lib, workloads  # noqa: E402
from plato_amd.arena import ArenaLayout  # noqa: E402
from plato_amd.engine import ClientSlab, DeviceArena, FedAvgEngine, fedavg_weights, fp32_weights  # noqa: E402
from plato_amd.krum import bulyan_select  # noqa: E402
from plato_amd.synthetic import fill_baseline, fill_clients  # noqa: E402

F = 3
MEDIAN, NEAREST = _lib.PLATO_AGG_ROBUST["median"], _lib.PLATO_AGG_ROBUST["nearest_mean"]


def device_part(k: int, reps: int, layout, dev):
    engine = FedAvgEngine(dev)
    base, slab = DeviceArena(layout, dev), ClientSlab(layout, k, dev)
    fill_baseline(base, 23)
    fill_clients(slab, base, 23, k)
    pf, pi = slab.row_pointers(range(k))
    tf, ti = torch.from_numpy(pf).to(dev), torch.from_numpy(pi).to(dev)
    n_f, n_i = layout.n_f32, layout.n_i64
    stream = torch.cuda.current_stream(dev)
    sh = stream.cuda_stream
    work = torch.empty(_lib.lib().plato_agg_pairwise_sqdist_workspace(k, n_f, n_i), dtype=torch.uint8, device=dev)
    dist = torch.empty((k, k), dtype=torch.float64, device=dev)
    out_f = torch.empty(layout.row_f32, dtype=torch.float32, device=dev)
    out_i = torch.empty(layout.row_i64, dtype=torch.float32, device=dev)
    w = torch.from_numpy(fp32_weights(fedavg_weights([1000] * k))).to(dev)

    def sqdist():
        _lib.call("plato_agg_pairwise_sqdist", tf.data_ptr(), ti.data_ptr(), k, n_f, n_i, work.data_ptr(),
                  dist.data_ptr(), sh)

    sqdist()
    torch.cuda.synchronize()
    host = dist.cpu().numpy()
    select_ms = []
    for _ in range(5):
        t0 = time.perf_counter()
        sel = bulyan_select(host, F)
        select_ms.append((time.perf_counter() - t0) * 1e3)
    spf, spi = slab.row_pointers(sel)
    sf, si = torch.from_numpy(spf).to(dev), torch.from_numpy(spi).to(dev)

    def columns(mode, trim, rows_f=tf, rows_i=ti, rows=k):
        return lambda: _lib.call("plato_agg_robust_columns", mode, rows_f.data_ptr(), rows_i.data_ptr(), rows, trim,
                                 out_f.data_ptr(), out_i.data_ptr(), n_f, n_i, sh)

    def fedavg():
        engine.launch_fedavg(layout, tf, ti, w, None, k, base.f32, base.i64, out_f, out_i, stream)

    kernels = {"robust_median": columns(MEDIAN, 0), "nearest_mean trim 0": columns(NEAREST, 0),
               f"nearest_mean trim {F}": columns(NEAREST, F), "bulyan: pairwise_sqdist": sqdist,
               f"bulyan: nearest_mean theta={len(sel)}": columns(NEAREST, F, sf, si, len(sel)), "fedavg": fedavg}
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
    print(f"K={k} D={n_f + n_i} reps={reps} f={F} theta={len(sel)}")
    med = {name: statistics.median(a.elapsed_time(b) for a, b in evs) for name, evs in events.items()}
    for name, evs in events.items():
        ms = [a.elapsed_time(b) for a, b in evs]
        rows = len(sel) if "theta" in name else k + (name == "fedavg")
        gb = (rows * (n_f * 4 + n_i * 8) + (n_f + n_i) * 4) / 1e9  # every row once, the result once
        line = f"  {name:34s} median {med[name]:9.3f} ms   min {min(ms):9.3f} ms"
        if "sqdist" not in name:
            line += f"   {gb / med[name] * 1e3:8.1f} GB/s"
        if "nearest_mean" in name:
            line += f"   {med[name] / med['robust_median']:.2f} x robust_median"
        print(line)
    print(f"  {'bulyan: host selection':34s} median {statistics.median(select_ms):9.3f} ms   min {min(select_ms):9.3f} ms")
    sys.stdout.flush()
    del slab, base, work
    torch.cuda.empty_cache()


def host_part(k: int, layout):
    """aggregations.trimmed_mean's op sequence after flatten_weights, on the CPU."""
    from oracle import synth

    n = layout.n_f32 + layout.n_i64
    bf, bi = synth.baseline_arena(layout.n_f32, layout.n_i64, 23)
    rows = []
    for c in range(k):
        xf, xi = synth.client_arena(bf, bi, 23, c)
        rows.append(torch.cat((torch.from_numpy(xf), torch.from_numpy(xi))))  # promotes the counters, as flatten_weights
    x = torch.stack(rows)
    assert x.shape == (k, n) and x.dtype == torch.float32
    for trim in (0, F):
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            med = torch.median(x, dim=0)[0]
            idx = torch.argsort(torch.abs(x - med), dim=0)
            srt = x[idx, torch.arange(n)[None, :]]
            torch.mean(srt[: k - 2 * trim], dim=0)
            times.append(time.perf_counter() - t0)
        print(f"host K={k} D={n} trim={trim} threads={torch.get_num_threads()}: median, argsort, gather, mean "
              f"median {statistics.median(times) * 1e3:.1f} ms  min {min(times) * 1e3:.1f} ms")
        sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="128,256")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-ks", default="16,32")
    args = ap.parse_args()
    layout = ArenaLayout.from_shapes(workloads.resnet(18, 10))
    if args.ks:
        if not torch.cuda.is_available():
            raise SystemExit("bench_bulyan: no GPU (the device part measures nothing without one)")
        dev = torch.device("cuda:0")
        print(torch.cuda.get_device_name(0))
        for k in (int(v) for v in args.ks.split(",")):
            device_part(k, args.reps, layout, dev)
    if args.host_ks:
        torch.set_num_threads(16)
        for k in (int(v) for v in args.host_ks.split(",")):
            host_part(k, layout)


if __name__ == "__main__":
    main()
