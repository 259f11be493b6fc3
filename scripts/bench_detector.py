"""FLDetector's kernels at K x ResNet-18 with a record of N rounds, HIP events, interleaved in one process
(DESIGN.md §25).

    python scripts/bench_detector.py [--ks 16,128] [--ns 1,16,64] [--reps 10]

Per (K, N) the four kernels of a round and plato_agg_mean_rows over the same K rows (the project's streaming
yardstick) run in turn in every repetition, after a warm-up of every shape; median and minimum over the
repetitions.  Each kernel's line has its time as a multiple of mean_rows' and its achieved GB/s over the
bytes it has to move:

    mean_rows        K client rows read, one fp32 row written
    detect_means     K client rows, the baseline and two flat rows read, five flat rows written
    rows_dots        2N + 2 flat rows read once, three vectors (re-read once per batch of 8 rows, from L2)
    lbfgs_predict    2N flat rows and two more read, one written
    delta_sqdist     K client rows read, the baseline and the prediction once per batch of 8 clients

The host part of a round (the 2N x 2N solve, the scores, the split) is timed beside them.
"""

from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from plato_amd import _lib, detectors, workloads  # noqa: E402
from plato_amd.arena import ArenaLayout  # noqa: E402
from plato_amd.engine import ClientSlab, DeviceArena  # noqa: E402
from plato_amd.synthetic import fill_baseline, fill_clients  # noqa: E402

HBM_BYTES_PER_S = 6.29e12  # MI355X HBM3E as measured by a float4 copy


def run(k: int, n: int, reps: int, layout, dev):
    n_f, n_i = layout.n_f32, layout.n_i64
    d = n_f + n_i
    base, slab = DeviceArena(layout, dev), ClientSlab(layout, k, dev)
    fill_baseline(base, 23)
    fill_clients(slab, base, 23, k)
    stream = torch.cuda.current_stream(dev)
    sh = stream.cuda_stream
    pf, pi = slab.row_pointers(range(k))
    tf, ti = torch.from_numpy(pf).to(dev), torch.from_numpy(pi).to(dev)
    r = 2 * n
    record = torch.randn((r + 2, d), dtype=torch.float32, device=dev) * 0.01   # S, Y, then s_new, y_new
    flat = torch.randn((7, d), dtype=torch.float32, device=dev) * 0.01         # last_w, last_g, g, v, b_flat, pred, spare
    last_w, last_g, g, v, b_flat, pred, _ = flat
    rows = torch.tensor([record[j].data_ptr() for j in range(r + 2)], dtype=torch.int64, device=dev)
    vecs = torch.tensor([v.data_ptr(), record[r].data_ptr(), record[r + 1].data_ptr()], dtype=torch.int64, device=dev)
    a = torch.randn(r, dtype=torch.float64, device=dev)
    lib = _lib.lib()
    work_dots = torch.empty(lib.plato_agg_rows_dots_workspace(r + 2, 3, d), dtype=torch.uint8, device=dev)
    work_dist = torch.empty(lib.plato_agg_delta_sqdist_workspace(k, n_f, n_i), dtype=torch.uint8, device=dev)
    dots = torch.empty((r + 2, 3), dtype=torch.float64, device=dev)
    d2 = torch.empty(k, dtype=torch.float64, device=dev)
    out_f = torch.empty(layout.row_f32, dtype=torch.float32, device=dev)
    out_i = torch.empty(layout.row_i64, dtype=torch.float32, device=dev)

    kernels = {
        "mean_rows": lambda: _lib.call("plato_agg_mean_rows", tf.data_ptr(), ti.data_ptr(), k, out_f.data_ptr(),
                                       out_i.data_ptr(), n_f, n_i, sh),
        "detect_means": lambda: _lib.call("plato_agg_detect_means", tf.data_ptr(), ti.data_ptr(), k, base.f32.data_ptr(),
                                          base.i64.data_ptr(), last_w.data_ptr(), last_g.data_ptr(), g.data_ptr(),
                                          v.data_ptr(), record[r].data_ptr(), record[r + 1].data_ptr(), b_flat.data_ptr(),
                                          n_f, n_i, sh),
        "rows_dots": lambda: _lib.call("plato_agg_rows_dots", rows.data_ptr(), r + 2, vecs.data_ptr(), 3, d,
                                       work_dots.data_ptr(), dots.data_ptr(), sh),
        "lbfgs_predict": lambda: _lib.call("plato_agg_lbfgs_predict", rows.data_ptr(), r, a.data_ptr(), 0.75,
                                           last_g.data_ptr(), v.data_ptr(), pred.data_ptr(), d, sh),
        "delta_sqdist": lambda: _lib.call("plato_agg_delta_sqdist", tf.data_ptr(), ti.data_ptr(), k, base.f32.data_ptr(),
                                          base.i64.data_ptr(), pred.data_ptr(), n_f, n_i, work_dist.data_ptr(),
                                          d2.data_ptr(), sh),
    }
    row_bytes, base_bytes = n_f * 4 + n_i * 8, n_f * 4 + n_i * 8
    batches = -(-k // 8)
    gb = {"mean_rows": (k * row_bytes + d * 4) / 1e9,
          "detect_means": (k * row_bytes + base_bytes + 7 * d * 4) / 1e9,
          "rows_dots": (r + 2) * d * 4 / 1e9,
          "lbfgs_predict": (r + 3) * d * 4 / 1e9,
          "delta_sqdist": (k * row_bytes + batches * (base_bytes + d * 4)) / 1e9}
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
    times = {name: [e0.elapsed_time(e1) for e0, e1 in evs] for name, evs in events.items()}
    med = {name: statistics.median(ms) for name, ms in times.items()}
    print(f"K={k} N={n} D={d} reps={reps} record_GB={(r + 2) * d * 4 / 1e9:.2f} "
          f"HBM floor of the K rows {k * row_bytes / HBM_BYTES_PER_S * 1e3:.3f} ms")
    for name, ms in times.items():
        rate = gb[name] / med[name] * 1e3
        print(f"  {name:14s} median {med[name]:9.3f} ms   min {min(ms):9.3f} ms   max {max(ms):9.3f} ms   "
              f"{med[name] / med['mean_rows']:6.2f} x mean_rows   {rate:8.1f} GB/s   "
              f"{rate / (gb['mean_rows'] / med['mean_rows'] * 1e3):.2f} x mean_rows' rate")
    # the host's part on a well-conditioned system of the same size
    rng = np.random.default_rng(1)
    s, y = rng.standard_normal((n, 4 * n + 8)), rng.standard_normal((n, 4 * n + 8))
    y = 0.8 * s + 0.05 * y
    vv = rng.standard_normal(4 * n + 8)
    sy, ss, yy = s @ y.T, s @ s.T, float(y[-1] @ y[-1])
    host = []
    for _ in range(5):
        t0 = time.perf_counter()
        detectors.lbfgs_coefficients(sy, ss, yy, s @ vv, y @ vv)
        scores = detectors.normalised_distances(rng.uniform(1, 2, k))
        detectors.two_means_1d(scores)
        host.append((time.perf_counter() - t0) * 1e3)
    print(f"  host (solve of {2 * n} x {2 * n}, scores, split) median {statistics.median(host):.3f} ms")
    sys.stdout.flush()
    del slab, base, record, flat, kernels
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="16,128")
    ap.add_argument("--ns", default="1,16,64")
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_detector: no GPU (it measures nothing without one)")
    layout = ArenaLayout.from_shapes(workloads.resnet(18, 10))
    dev = torch.device("cuda:0")
    print(torch.cuda.get_device_name(0))
    for k in (int(v) for v in args.ks.split(",")):
        for n in (int(v) for v in args.ns.split(",")):
            run(k, n, args.reps, layout, dev)


if __name__ == "__main__":
    main()
