"""plato_agg_elastic_mean on one GPU, HIP events.

    python scripts/bench_elastic.py [--k 128] [--reps 20] [--warmup 3] [--blocks 5] [--only w1|w2]

W1, width only: §22's workload (``workloads.resnet(18)`` shapes, the ``weight`` / ``bias`` entries, client c at
rate 1, 1/2, 1/4, 1/8, 1/16 in turn).  ``plato_agg_submodel_mean`` and ``plato_agg_elastic_mean`` run on the same
global region and the same client rows, turn by turn, in ``--blocks`` blocks of ``--reps`` timed pairs; the two
outputs are compared bit for bit.  Reported: both medians, the block medians, and the spread of the old
kernel's block medians.

W2, depth and width: the global model has the shapes of the reference's ``ResnetWrapper`` at depths [3, 4, 6, 3]
and rate 1; client c draws each stage's depth from 2..max and each stage's width from {0.5, 1} (seeded).  In
the same process, turn by turn with it, ``plato_agg_mean_rows`` runs over K full rows of the same model: the
streaming yardstick.  Reported: time, bytes, GB/s, the fraction of ``mean_rows``' rate, and the share of
(entry, client) pairs without a box.

Rows and tables are built on the device and by ``plato_amd.elastic.build_tables``; nothing is staged from the
host, so the figures are the kernels'.  Prints one JSON line per workload.

    bytes = 4 * (2 * N_entries + sum of the boxes)   (global read, result written, every box read once)
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
from plato_amd import elastic as el  # noqa: E402
from plato_amd import submodel as sm  # noqa: E402
from plato_amd.arena import ArenaLayout  # noqa: E402
from plato_amd.engine import ClientSlab, DeviceArena  # noqa: E402
from plato_amd.synthetic import BASE_SCALE, CLIENT_SCALE, fill_baseline, fill_clients  # noqa: E402

RATES = (1.0, 0.5, 0.25, 0.125, 0.0625)
HIDDEN = (64, 128, 256, 512)
DEPTHS = (3, 4, 6, 3)


def client_shape(shape, rank: int, rate: float):
    """The leading ``rank`` dims that are hidden widths scaled by ``rate`` (image channels and classes stay)."""
    return tuple(int(np.ceil(rate * d)) if i < rank and d in HIDDEN else d for i, d in enumerate(shape))


def wrapper_spec(depths, rates):
    """(name, shape, region) of the reference's sysheterofl ResnetWrapper(configs=[depths, rates])."""
    hidden = [int(np.ceil(r * x)) for r, x in zip(rates, HIDDEN)]

    def bn(p, c):
        return [(p + ".weight", (c,), "f32"), (p + ".bias", (c,), "f32"), (p + ".running_mean", (c,), "f32"),
                (p + ".running_var", (c,), "f32"), (p + ".num_batches_tracked", (), "i64")]

    spec, inp = [("model.conv1.weight", (hidden[0], 3, 3, 3), "f32")], hidden[0]
    for layer, (planes, stride, blocks) in enumerate(zip(hidden, (1, 2, 2, 2), depths), start=1):
        for block in range(blocks):
            p = f"model.layer{layer}.{block}"
            spec += bn(p + ".batchnorm1", inp) + [(p + ".conv1.weight", (planes, inp, 3, 3), "f32")]
            spec += bn(p + ".batchnorm2", planes) + [(p + ".conv2.weight", (planes, planes, 3, 3), "f32")]
            if (stride if block == 0 else 1) != 1 or inp != planes:
                spec.append((p + ".shortcut.weight", (planes, inp, 1, 1), "f32"))
            inp = planes
    return spec + bn("model.bn4", hidden[3]) + [("model.linear.weight", (10, hidden[3]), "f32"),
                                                ("model.linear.bias", (10,), "f32")]


class Buffers:
    """The global region, the clients' compact rows back to back (256-byte aligned) and an output, on the device."""

    def __init__(self, n: int, row_len: np.ndarray, dev, sh):
        self.n, k = n, len(row_len)
        self.d_global = torch.empty(n, dtype=torch.float32, device=dev)
        _lib.call("plato_agg_fill_synth_f32", self.d_global.data_ptr(), None, n, 23, 0, BASE_SCALE, sh)
        offs = np.concatenate([[0], np.cumsum(-(-row_len // 64) * 64)])
        self.slab = torch.empty(max(int(offs[-1]), 1), dtype=torch.float32, device=dev)
        for c in range(k):
            if row_len[c]:
                _lib.call("plato_agg_fill_synth_f32", self.slab.data_ptr() + 4 * int(offs[c]), None, int(row_len[c]), 23,
                          c + 1, CLIENT_SCALE, sh)
        self.rows = torch.from_numpy((self.slab.data_ptr() + 4 * offs[:-1]).astype(np.int64)).to(dev)


def elastic_call(buf: Buffers, tab: el.ElasticTables, out, dev, sh):
    d_tables = torch.empty(_lib.lib().plato_agg_elastic_tables_bytes(len(tab.entries), len(tab.boxes)),
                           dtype=torch.uint8, device=dev)
    h_entries, h_boxes = torch.from_numpy(tab.entries).pin_memory(), torch.from_numpy(tab.boxes).pin_memory()

    def call():
        _lib.call("plato_agg_elastic_mean", buf.d_global.data_ptr(), buf.rows.data_ptr(), tab.k, tab.row_len.ctypes.data,
                  h_entries.data_ptr(), len(tab.entries), h_boxes.data_ptr(), len(tab.boxes), d_tables.data_ptr(),
                  out.data_ptr(), buf.n, sh)

    call.keep = (d_tables, h_entries, h_boxes)
    return call


def timed_blocks(kernels: dict, stream, warmup: int, reps: int, blocks: int) -> dict:
    """name -> [[ms] per block]: the kernels turn by turn, ``reps`` timed rounds per block."""
    for _ in range(warmup):
        for fn in kernels.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in kernels}
    for _ in range(blocks):
        events = {name: [] for name in kernels}
        for _ in range(reps):
            for name, fn in kernels.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                events[name].append((e0, e1))
        torch.cuda.synchronize()
        for name, evs in events.items():
            ms[name].append([e0.elapsed_time(e1) for e0, e1 in evs])
    return ms


def summary(blocks: list) -> dict:
    flat = [v for b in blocks for v in b]
    meds = [statistics.median(b) for b in blocks]
    return {"ms_median": round(statistics.median(flat), 4), "ms_min": round(min(flat), 4), "ms_max": round(max(flat), 4),
            "block_medians": [round(m, 4) for m in meds], "block_spread_ms": round(max(meds) - min(meds), 4)}


def w1(args, dev, stream):
    sh, k = stream.cuda_stream, args.k
    glayout = ArenaLayout.from_shapes([(n, s, r) for n, s, r in workloads.resnet(18, 10) if sm.participates(n)])
    sigs = []
    for c in range(k):
        rate = RATES[c % len(RATES)]
        sigs.append(tuple((e.name, client_shape(e.shape, sm.prefix_rank("heterofl", e.name, len(e.shape)), rate))
                          for e in glayout.entries if sm.prefix_rank("heterofl", e.name, len(e.shape))))
    old, new = sm.build_tables(glayout, sigs, "heterofl"), el.build_tables(glayout, sigs)
    assert (old.row_len == new.row_len).all() and old.covered() == new.covered() and old.n_out == new.n_out
    buf = Buffers(old.n_out, old.row_len, dev, sh)
    out_old = torch.empty(buf.n, dtype=torch.float32, device=dev)
    out_new = torch.empty(buf.n, dtype=torch.float32, device=dev)
    d_tables = torch.empty(_lib.lib().plato_agg_submodel_tables_bytes(k, len(old.entries)), dtype=torch.uint8, device=dev)
    h_entries, h_boxes = torch.from_numpy(old.entries).pin_memory(), torch.from_numpy(old.boxes).pin_memory()

    def submodel_mean():
        _lib.call("plato_agg_submodel_mean", buf.d_global.data_ptr(), buf.rows.data_ptr(), k, old.row_len.ctypes.data,
                  h_entries.data_ptr(), h_boxes.data_ptr(), len(old.entries), d_tables.data_ptr(), out_old.data_ptr(),
                  buf.n, sh)

    ms = timed_blocks({"submodel_mean": submodel_mean, "elastic_mean": elastic_call(buf, new, out_new, dev, sh)},
                      stream, args.warmup, args.reps, args.blocks)
    same = bool((out_old.view(torch.int32) == out_new.view(torch.int32)).all())
    s_old, s_new = summary(ms["submodel_mean"]), summary(ms["elastic_mean"])
    nbytes = new.algorithmic_bytes()
    print(json.dumps({
        "bench": "elastic_mean", "workload": "w1_width_only", "device": torch.cuda.get_device_name(0), "k": k,
        "reps": args.reps, "warmup": args.warmup, "blocks": args.blocks, "rates": list(RATES),
        "n_entries_elements": int(buf.n), "covered": new.covered(), "bytes": nbytes, "boxes": len(new.boxes),
        "outputs_equal_bitwise": same,
        "submodel_mean": dict(s_old, GBps=round(nbytes / s_old["ms_median"] / 1e6, 1)),
        "elastic_mean": dict(s_new, GBps=round(nbytes / s_new["ms_median"] / 1e6, 1)),
        "elastic_over_submodel": round(s_new["ms_median"] / s_old["ms_median"], 4),
        "difference_ms": round(s_new["ms_median"] - s_old["ms_median"], 4),
    }), flush=True)
    if not same:
        raise SystemExit("bench_elastic: the two kernels differ on the width-only workload")


def w2(args, dev, stream):
    sh, k = stream.cuda_stream, args.k
    spec = wrapper_spec(DEPTHS, (1.0,) * 4)
    full = ArenaLayout.from_shapes(spec)
    glayout = ArenaLayout.from_shapes([(n, s, r) for n, s, r in spec if r == "f32"])
    rng = np.random.default_rng(23)
    sigs = []
    for _ in range(k):
        depths = [int(rng.integers(2, d + 1)) for d in DEPTHS]
        rates = [float(rng.choice([0.5, 1.0])) for _ in DEPTHS]
        sigs.append(tuple((n, s) for n, s, r in wrapper_spec(depths, rates) if r == "f32" and el.rank_of(n, len(s))))
    tab = el.build_tables(glayout, sigs)
    buf = Buffers(tab.n_out, tab.row_len, dev, sh)
    out = torch.empty(buf.n, dtype=torch.float32, device=dev)

    # the yardstick: K full rows of the same model through plato_agg_mean_rows
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

    ms = timed_blocks({"elastic_mean": elastic_call(buf, tab, out, dev, sh), "mean_rows": mean_rows}, stream,
                      args.warmup, args.reps, 1)
    s_new, s_wide = summary(ms["elastic_mean"]), summary(ms["mean_rows"])
    nbytes = tab.algorithmic_bytes()
    wide_bytes = k * (full.n_f32 * 4 + full.n_i64 * 8) + (full.n_f32 + full.n_i64) * 4
    gbps, wide_gbps = nbytes / s_new["ms_median"] / 1e6, wide_bytes / s_wide["ms_median"] / 1e6
    print(json.dumps({
        "bench": "elastic_mean", "workload": "w2_depth_and_width", "device": torch.cuda.get_device_name(0), "k": k,
        "reps": args.reps, "warmup": args.warmup, "depths": list(DEPTHS), "width_rates": [0.5, 1.0],
        "n_entries": len(tab.entries), "n_entries_elements": int(buf.n), "covered": tab.covered(), "bytes": nbytes,
        "boxes": len(tab.boxes), "absent_pair_share": round(tab.absent_share(), 4),
        "ms_median": s_new["ms_median"], "ms_min": s_new["ms_min"], "ms_max": s_new["ms_max"], "GBps": round(gbps, 1),
        "mean_rows_bytes": wide_bytes, "mean_rows_ms_median": s_wide["ms_median"], "mean_rows_ms_min": s_wide["ms_min"],
        "mean_rows_GBps": round(wide_gbps, 1), "fraction_of_mean_rows_rate": round(gbps / wide_gbps, 3),
    }), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--only", choices=("w1", "w2"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_elastic: no GPU (it measures nothing without one)")
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    if args.only != "w2":
        w1(args, dev, stream)
    if args.only != "w1":
        w2(args, dev, stream)


if __name__ == "__main__":
    main()
