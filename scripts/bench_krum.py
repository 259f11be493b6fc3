"""Multi-Krum's pieces at K x ResNet-18, HIP events, interleaved in one process.

    python scripts/bench_krum.py [--ks 128,256] [--reps 10] [--host-ks 16,32]

Per K: plato_agg_pairwise_sqdist, plato_agg_mean_rows over the K - 6 selected rows, the fused FedAvg kernel
on the same rows (the streaming yardstick), and the host selection (plato_amd.krum) on the device's
matrix.  Each repetition runs the three kernels in turn; median and minimum over the repetitions.
Floors of the distance kernel from the MI355X's vector rate and HBM bandwidth are printed beside it.

--host-ks: the reference's own op sequence on this host's CPU at 16 threads, one selection step's distance
loop (`torch.norm(X - X[i], dim=1) ** 2` for each i, aggregations.py:186-192) on the same synthetic rows.
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
from plato_amd.krum import multi_krum_select  # noqa: E402
from plato_amd.synthetic import fill_baseline, fill_clients  # noqa: E402

# MI355X: 256 CUs x 4 SIMDs x 32 lanes per clock at 2.4 GHz; HBM3E as measured by a float4 copy
LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9
HBM_BYTES_PER_S = 6.29e12
TILE = 32


def floors(k: int, d: int):
    pairs = k * (k - 1) // 2
    valu_ms = pairs * d * 2 / LANE_OPS_PER_S * 1e3          # one v_sub_f32 and one v_fma_f32 per pair and coordinate
    hbm_ms = k * d * 4 / HBM_BYTES_PER_S * 1e3               # every row once
    t = -(-k // TILE)
    tiled_gb = t * (t + 1) // 2 * 2 * TILE * d * 4 / 1e9     # 64 rows per 32 x 32 tile (mostly L2 / Infinity Cache hits)
    return valu_ms, hbm_ms, tiled_gb


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
        sel = multi_krum_select(host, 2)
        select_ms.append((time.perf_counter() - t0) * 1e3)
    spf, spi = slab.row_pointers(sel)
    sf, si = torch.from_numpy(spf).to(dev), torch.from_numpy(spi).to(dev)

    def mean():
        _lib.call("plato_agg_mean_rows", sf.data_ptr(), si.data_ptr(), len(sel), out_f.data_ptr(), out_i.data_ptr(),
                  n_f, n_i, sh)

    def fedavg():
        engine.launch_fedavg(layout, tf, ti, w, None, k, base.f32, base.i64, out_f, out_i, stream)

    kernels = {"pairwise_sqdist": sqdist, "mean_rows": mean, "fedavg": fedavg}
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
    d = n_f + n_i
    valu_ms, hbm_ms, tiled_gb = floors(k, d)
    print(f"K={k} D={d} reps={reps} selected={len(sel)} workspace_MB={work.numel() / 1e6:.1f}")
    for name, evs in events.items():
        ms = [a.elapsed_time(b) for a, b in evs]
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
    sys.stdout.flush()
    del slab, base, work
    torch.cuda.empty_cache()


def host_part(k: int, layout):
    """One selection step's distance loop of the reference, on the CPU."""
    from oracle import synth

    n = layout.n_f32 + layout.n_i64
    bf, bi = synth.baseline_arena(layout.n_f32, layout.n_i64, 23)
    rows = []
    for c in range(k):
        xf, xi = synth.client_arena(bf, bi, 23, c)
        rows.append(torch.cat((torch.from_numpy(xf), torch.from_numpy(xi))))  # promotes the counters, as flatten_weights
    x = torch.stack(rows)
    assert x.shape == (k, n) and x.dtype == torch.float32
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        for weight in x:
            torch.norm((x - weight), dim=1) ** 2
        times.append(time.perf_counter() - t0)
    print(f"host K={k} D={n} threads={torch.get_num_threads()}: one step's distance loop "
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
            raise SystemExit("bench_krum: no GPU (the device part measures nothing without one)")
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
