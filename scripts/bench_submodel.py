"""plato_agg_submodel_mean at K x ResNet-18 sub-models, HIP events.

    python scripts/bench_submodel.py [--k 128] [--reps 20] [--warmup 3] [--rule heterofl]

The global model has the shapes of ``workloads.resnet(18)``; client c has every hidden width (64, 128, 256,
512) scaled by ``ceil(rate * width)`` with the rates 1, 1/2, 1/4, 1/8, 1/16 taken in turn.  Rows and tables
are built on the device and by ``plato_amd.submodel.build_tables``; nothing is staged from the host, so the
figure is the kernel's.  In the same process, turn by turn with it, ``plato_agg_mean_rows`` runs over K
full-width rows of the same model: the streaming yardstick.  Prints one JSON line.

    bytes = 4 * (2 * N_participating + sum_k covered_k)   (global read, result written, every box read once)
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from plato_amd import _lib, workloads  # noqa: E402
from plato_amd import submodel as sm  # noqa: E402
from plato_amd.arena import ArenaLayout  # noqa: E402
from plato_amd.engine import ClientSlab, DeviceArena  # noqa: E402
from plato_amd.synthetic import BASE_SCALE, CLIENT_SCALE, fill_baseline, fill_clients  # noqa: E402

RATES = (1.0, 0.5, 0.25, 0.125, 0.0625)
HIDDEN = (64, 128, 256, 512)


def client_shape(shape, rank: int, rate: float):
    """The leading ``rank`` dims that are hidden widths scaled by ``rate`` (image channels and classes stay)."""
    return tuple(int(np.ceil(rate * d)) if i < rank and d in HIDDEN else d for i, d in enumerate(shape))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rule", default="heterofl", choices=sorted(sm.RULES))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_submodel: no GPU (it measures nothing without one)")
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    sh, k = stream.cuda_stream, args.k

    full = ArenaLayout.from_shapes(workloads.resnet(18, 10))
    glayout = ArenaLayout.from_shapes([(n, s, r) for n, s, r in workloads.resnet(18, 10) if sm.participates(n)])
    sigs = []
    for c in range(k):
        rate = RATES[c % len(RATES)]
        sigs.append(tuple((e.name, client_shape(e.shape, sm.prefix_rank(args.rule, e.name, len(e.shape)), rate))
                          for e in glayout.entries if sm.prefix_rank(args.rule, e.name, len(e.shape))))
    tab = sm.build_tables(glayout, sigs, args.rule)

    # device buffers: the global region, the clients' compact rows back to back (256-byte aligned), the output
    n = tab.n_out
    d_global = torch.empty(n, dtype=torch.float32, device=dev)
    _lib.call("plato_agg_fill_synth_f32", d_global.data_ptr(), None, n, 23, 0, BASE_SCALE, sh)
    offs = np.concatenate([[0], np.cumsum(-(-tab.row_len // 64) * 64)])
    slab = torch.empty(int(offs[-1]), dtype=torch.float32, device=dev)
    for c in range(k):
        if tab.row_len[c]:
            _lib.call("plato_agg_fill_synth_f32", slab.data_ptr() + 4 * int(offs[c]), None, int(tab.row_len[c]), 23,
                      c + 1, CLIENT_SCALE, sh)
    rows = torch.from_numpy((slab.data_ptr() + 4 * offs[:-1]).astype(np.int64)).to(dev)
    out = torch.empty(n, dtype=torch.float32, device=dev)
    d_tables = torch.empty(_lib.lib().plato_agg_submodel_tables_bytes(k, len(tab.entries)), dtype=torch.uint8, device=dev)
    h_entries, h_boxes = torch.from_numpy(tab.entries).pin_memory(), torch.from_numpy(tab.boxes).pin_memory()

    def submodel_mean():
        _lib.call("plato_agg_submodel_mean", d_global.data_ptr(), rows.data_ptr(), k, tab.row_len.ctypes.data,
                  h_entries.data_ptr(), h_boxes.data_ptr(), len(tab.entries), d_tables.data_ptr(), out.data_ptr(), n, sh)

    # the yardstick: K full-width rows of the same model through plato_agg_mean_rows
    base, wide = DeviceArena(full, dev), ClientSlab(full, k, dev)
    fill_baseline(base, 23)
    fill_clients(wide, base, 23, k)
    pf, pi = wide.row_pointers(range(k))
    tf, ti = torch.from_numpy(pf).to(dev), torch.from_numpy(pi).to(dev)
    out_f = torch.empty(full.row_f32, dtype=torch.float32, device=dev)
    out_i = torch.empty(full.row_i64, dtype=torch.float32, device=dev)

    def mean_rows():
        _lib.call("plato_agg_mean_rows", tf.data_ptr(), ti.data_ptr(), k, out_f.data_ptr(), out_i.data_ptr(),
                  full.n_f32, full.n_i64, sh)

    kernels = {"submodel_mean": submodel_mean, "mean_rows": mean_rows}
    for _ in range(args.warmup):
        for fn in kernels.values():
            fn()
    torch.cuda.synchronize()
    events = {name: [] for name in kernels}
    for _ in range(args.reps):
        for name, fn in kernels.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            events[name].append((e0, e1))
    torch.cuda.synchronize()
    ms = {name: [e0.elapsed_time(e1) for e0, e1 in evs] for name, evs in events.items()}
    med = {name: statistics.median(v) for name, v in ms.items()}
    nbytes = tab.algorithmic_bytes()
    wide_bytes = k * (full.n_f32 * 4 + full.n_i64 * 8) + (full.n_f32 + full.n_i64) * 4
    gbps = nbytes / med["submodel_mean"] / 1e6
    wide_gbps = wide_bytes / med["mean_rows"] / 1e6
    print(json.dumps({
        "bench": "submodel_mean", "device": torch.cuda.get_device_name(0), "rule": args.rule, "k": k,
        "reps": args.reps, "warmup": args.warmup, "rates": list(RATES),
        "n_participating": int(n), "covered": tab.covered(), "bytes": nbytes,
        "ms_median": round(med["submodel_mean"], 4), "ms_min": round(min(ms["submodel_mean"]), 4),
        "ms_max": round(max(ms["submodel_mean"]), 4), "GBps": round(gbps, 1),
        "mean_rows_bytes": wide_bytes, "mean_rows_ms_median": round(med["mean_rows"], 4),
        "mean_rows_ms_min": round(min(ms["mean_rows"]), 4), "mean_rows_GBps": round(wide_gbps, 1),
        "fraction_of_mean_rows_rate": round(gbps / wide_gbps, 3),
    }))


if __name__ == "__main__":
    main()
