"""Global magnitude pruning at ResNet-18's prunable size, HIP events, interleaved in one process
(DESIGN.md §26).

    python scripts/bench_prune.py [--amounts 0.2,0.8] [--reps 20]

Per amount, in every repetition in turn, after a warm-up of each:

    prune (dense)    plato_agg_prune_global over a row of random weights (restored before every repetition,
                     outside the timed span): 3 histogram reads, the masked read and write
    prune (pruned)   the same over the row it has just pruned, as a second call of the processor sees it: the
                     threshold is 0 with more zeros than k, so the read that ranks the ties runs as well
    mean_rows        plato_agg_mean_rows over one row of the same bytes (one read, one write): the project's
                     streaming yardstick

and once per amount the reference's selection on the host: torch.topk(|w|, k, largest=False) and w * mask.
Every line has its time as a multiple of mean_rows' and the bytes its passes move per second.
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

from plato_amd import _lib, workloads  # noqa: E402
from plato_amd import prune as host  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--amounts", default="0.2,0.8")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_prune: no GPU (it measures nothing without one)")
    dev = torch.device("cuda:0")
    print(torch.cuda.get_device_name(0))
    sizes = [int(np.prod(s)) for name, s, kind in workloads.resnet(18, 10)
             if kind == "f32" and name.endswith("weight") and len(s) in (2, 4)]
    n = sum(sizes)
    pieces, at = [], 0
    for s in sizes:
        pieces.append((at, at + s))
        at += s
    table = host.piece_table(pieces)
    weights = (np.random.default_rng(18).standard_normal(n) * 0.02).astype(np.float32)
    pristine = torch.from_numpy(weights).to(dev)
    row, pruned, out = torch.empty_like(pristine), torch.empty_like(pristine), torch.empty_like(pristine)
    lib = _lib.lib()
    work = torch.empty(lib.plato_agg_prune_global_workspace(len(table), n), dtype=torch.uint8, device=dev)
    result = torch.zeros(4, dtype=torch.int64, device=dev)
    ptr = torch.tensor([pristine.data_ptr()], dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev)
    sh = stream.cuda_stream
    print(f"n={n} pieces={len(pieces)} row_MB={n * 4 / 1e6:.1f} reps={args.reps}")

    def prune_call(target, k):
        _lib.call("plato_agg_prune_global", target.data_ptr(), n, table.ctypes.data, len(table), k, work.data_ptr(),
                  result.data_ptr(), sh)

    def mean_call():
        _lib.call("plato_agg_mean_rows", ptr.data_ptr(), None, 1, out.data_ptr(), None, n, 0, sh)

    for amount in (float(a) for a in args.amounts.split(",")):
        k = host.nparams_toprune(amount, n)
        pruned.copy_(pristine)
        prune_call(pruned, k)
        dense_rec = result.cpu().tolist()
        again = pruned.clone()
        prune_call(again, k)
        pruned_rec = result.cpu().tolist()
        assert torch.equal(again.view(torch.int32), pruned.view(torch.int32))  # the second call changes no bit
        del again
        calls = {"prune (dense)": lambda: prune_call(row, k), "prune (pruned)": lambda: prune_call(pruned, k),
                 "mean_rows": mean_call}
        for fn in calls.values():
            row.copy_(pristine)
            fn()
        torch.cuda.synchronize()
        events = {name: [] for name in calls}
        for _ in range(args.reps):
            for name, fn in calls.items():
                row.copy_(pristine)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                events[name].append((e0, e1))
        torch.cuda.synchronize()
        times = {name: [e0.elapsed_time(e1) * 1e3 for e0, e1 in evs] for name, evs in events.items()}
        med = {name: statistics.median(us) for name, us in times.items()}
        # row passes: reads + writes
        passes = {"prune (dense)": 4 + 1 + (dense_rec[3] < dense_rec[2]),
                  "prune (pruned)": 4 + 1 + (pruned_rec[3] < pruned_rec[2]), "mean_rows": 2}
        print(f"amount={amount} k={k} dense T={dense_rec[0]:#010x} below={dense_rec[1]} ties={dense_rec[2]} r={dense_rec[3]}; "
              f"pruned T={pruned_rec[0]:#010x} ties={pruned_rec[2]} r={pruned_rec[3]}")
        for name, us in times.items():
            gbs = passes[name] * n * 4 / med[name] / 1e3
            print(f"  {name:15s} median {med[name]:9.1f} us   min {min(us):9.1f} us   max {max(us):9.1f} us   "
                  f"{med[name] / med['mean_rows']:6.2f} x mean_rows   {passes[name]} row passes   {gbs:8.1f} GB/s   "
                  f"{med[name] / (passes[name] / 2 * med['mean_rows']):.2f} x (passes x mean_rows / 2)")
        w = torch.from_numpy(weights)
        t0 = time.perf_counter()
        idx = torch.topk(w.abs(), k, largest=False).indices
        t1 = time.perf_counter()
        mask = torch.ones_like(w)
        mask[idx] = 0
        ref = w * mask
        t2 = time.perf_counter()
        print(f"  host reference   topk {1e3 * (t1 - t0):9.1f} ms   mask and multiply {1e3 * (t2 - t1):9.1f} ms")
        # the device's result against the host's where the answer is unique
        if dense_rec[3] == dense_rec[2]:
            pruned.copy_(pristine)
            prune_call(pruned, k)
            same = torch.equal(pruned.cpu().view(torch.int32), ref.view(torch.int32))
            print(f"  device row equals the host reference bit for bit: {same}")
        sys.stdout.flush()


if __name__ == "__main__":
    main()
