"""Fl-trust's pieces at K x ResNet-18, HIP events, interleaved in one process.

    python scripts/bench_fltrust.py [--ks 128,256] [--reps 10] [--host-ks 16,32]

Per K: plato_agg_mean_rows over the K rows, plato_agg_trust_stats against that mean, plato_agg_scaled_sum
with the scalars the statistics give (plato_amd.trust), and the fused FedAvg kernel on the same rows (the
streaming yardstick).  Each repetition runs the four kernels in turn; median and minimum over the
repetitions, the achieved GB/s of each (K rows read and one fp32 row besides: the result written, or the mean read)
and its ratio to mean_rows.  The HBM floor of one pass over the rows is printed beside them.

--host-ks: the reference's own op sequence on this host's CPU at 16 threads (aggregations.py:408-441:
torch.mean, the dot / norm loop, the clip, the candidates built by torch.cat and their torch.sum) on the
same synthetic rows, from the flattened matrix on (flatten_weights, quadratic in copies, is not timed).
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
from plato_amd.synthetic import fill_baseline, fill_clients  # noqa: E402
from plato_amd.trust import EPS, fltrust_weights  # noqa: E402

HBM_BYTES_PER_S = 6.29e12  # HBM3E as measured by a float4 copy


def device_part(k: int, reps: int, layout, dev):
    import numpy as np

    engine = FedAvgEngine(dev)
    base, slab = DeviceArena(layout, dev), ClientSlab(layout, k, dev)
    fill_baseline(base, 23)
    fill_clients(slab, base, 23, k)
    pf, pi = slab.row_pointers(range(k))
    tf, ti = torch.from_numpy(pf).to(dev), torch.from_numpy(pi).to(dev)
    n_f, n_i = layout.n_f32, layout.n_i64
    stream = torch.cuda.current_stream(dev)
    sh = stream.cuda_stream
    work = torch.empty(_lib.lib().plato_agg_trust_stats_workspace(k, n_f, n_i), dtype=torch.uint8, device=dev)
    stats = torch.empty(3 * k + 1, dtype=torch.float64, device=dev)
    mean_f = torch.empty(layout.row_f32, dtype=torch.float32, device=dev)
    mean_i = torch.empty(layout.row_i64, dtype=torch.float32, device=dev)
    out_f = torch.empty(layout.row_f32, dtype=torch.float32, device=dev)
    out_i = torch.empty(layout.row_i64, dtype=torch.float32, device=dev)
    w = torch.from_numpy(fp32_weights(fedavg_weights([1000] * k))).to(dev)

    def mean():
        _lib.call("plato_agg_mean_rows", tf.data_ptr(), ti.data_ptr(), k, mean_f.data_ptr(), mean_i.data_ptr(),
                  n_f, n_i, sh)

    def trust_stats():
        _lib.call("plato_agg_trust_stats", tf.data_ptr(), ti.data_ptr(), k, mean_f.data_ptr(), mean_i.data_ptr(), EPS,
                  n_f, n_i, work.data_ptr(), stats.data_ptr(), sh)

    mean()
    trust_stats()
    torch.cuda.synchronize()
    host_stats = stats.cpu().numpy()
    scalar_ms = []
    for _ in range(5):
        t0 = time.perf_counter()
        scal = fltrust_weights(host_stats, k, EPS)
        scalar_ms.append((time.perf_counter() - t0) * 1e3)
    table = torch.from_numpy(np.concatenate([scal["weights"], scal["div"]])).to(dev)

    def scaled_sum():
        _lib.call("plato_agg_scaled_sum", tf.data_ptr(), ti.data_ptr(), k, table.data_ptr(), table.data_ptr() + 4 * k,
                  float(scal["nm"]), out_f.data_ptr(), out_i.data_ptr(), n_f, n_i, sh)

    def fedavg():
        engine.launch_fedavg(layout, tf, ti, w, None, k, base.f32, base.i64, out_f, out_i, stream)

    kernels = {"mean_rows": mean, "trust_stats": trust_stats, "scaled_sum": scaled_sum, "fedavg": fedavg}
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
    row_bytes = n_f * 4 + n_i * 8
    floor_ms = k * row_bytes / HBM_BYTES_PER_S * 1e3
    print(f"K={k} D={d} reps={reps} workspace_MB={work.numel() / 1e6:.1f} clipped={int((scal['cos'] < 0).sum())} "
          f"HBM floor of one pass {floor_ms:.3f} ms")
    medians = {name: statistics.median([a.elapsed_time(b) for a, b in evs]) for name, evs in events.items()}
    for name, evs in events.items():
        ms = [a.elapsed_time(b) for a, b in evs]
        rows = k + 1 if name == "fedavg" else k
        gb = (rows * row_bytes + d * 4) / 1e9  # one fp32 row besides: the result written, or the mean read
        print(f"  {name:12s} median {medians[name]:9.3f} ms   min {min(ms):9.3f} ms   max {max(ms):9.3f} ms"
              f"   {gb / medians[name] * 1e3:8.1f} GB/s   {medians[name] / medians['mean_rows']:.2f} x mean_rows")
    total = medians["mean_rows"] + medians["trust_stats"] + medians["scaled_sum"]
    print(f"  Fl-trust kernels (mean_rows + trust_stats + scaled_sum) {total:9.3f} ms; host scalars "
          f"median {statistics.median(scalar_ms):.3f} ms")
    sys.stdout.flush()
    del slab, base, work
    torch.cuda.empty_cache()


def host_part(k: int, layout):
    """aggregations.fl_trust from the flattened matrix on, on the CPU."""
    from oracle import synth

    n = layout.n_f32 + layout.n_i64
    bf, bi = synth.baseline_arena(layout.n_f32, layout.n_i64, 23)
    rows = []
    for c in range(k):
        xf, xi = synth.client_arena(bf, bi, 23, c)
        rows.append(torch.cat((torch.from_numpy(xf), torch.from_numpy(xi))))  # promotes the counters, as flatten_weights
    flattened_weights = torch.stack(rows)
    assert flattened_weights.shape == (k, n) and flattened_weights.dtype == torch.float32
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
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
        times.append(time.perf_counter() - t0)
    print(f"host K={k} D={n} threads={torch.get_num_threads()}: fl_trust after flatten_weights "
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
            raise SystemExit("bench_fltrust: no GPU (the device part measures nothing without one)")
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
