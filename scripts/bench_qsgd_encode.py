"""The QSGD quantizer at ResNet-18's and ResNet-50's element counts, HIP events, interleaved in one process
(DESIGN.md §27).

    python scripts/bench_qsgd_encode.py [--models 18,50] [--reps 20] [--level 64]

Per model, in every repetition in turn, after a warm-up of each:

    encode           plato_agg_qsgd_encode over a device row of the model's state (one piece per entry): the
                     maxima (one read), the codes (one read, one byte written per element): 9 bytes per element
    mean_rows        plato_agg_mean_rows over one row of the same elements (one read, one write: 8 bytes per
                     element): the project's streaming yardstick
    encode_state_dict   the whole host call from CPU tensors (wall clock): staging, H2D, the kernels, the D2H copy
                     of codes and maxima, the headers and the bytes objects

Every line has its time as a multiple of mean_rows' and the bytes it moves per second.  The reference's own
time per element can only be taken on a CPU with the reference present; the figure quoted in DESIGN.md §27
was taken there, not here.
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
from plato_amd import qsgd_encode as host  # noqa: E402
from plato_amd.prune import piece_table  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="18,50")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--level", type=int, default=64)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_qsgd_encode: no GPU (it measures nothing without one)")
    dev = torch.device("cuda:0")
    print(torch.cuda.get_device_name(0))
    lib = _lib.lib()
    stream = torch.cuda.current_stream(dev)
    sh = stream.cuda_stream
    for depth in (int(d) for d in args.models.split(",")):
        spec = workloads.resnet(depth, 10)
        rng = np.random.default_rng(depth)
        state = {}
        for name, shape, kind in spec:
            n = int(np.prod(shape, dtype=np.int64))
            if kind == "f32":
                state[name] = torch.from_numpy((rng.standard_normal(n) * 0.02).astype(np.float32)).reshape(tuple(shape))
            else:
                state[name] = torch.from_numpy(rng.integers(1, 1000, n)).reshape(tuple(shape))
        pieces, at = [], 0
        for t in state.values():
            pieces.append((at, at + t.numel()))
            at += t.numel()
        n = at
        table = piece_table(pieces)
        row = torch.cat([t.reshape(-1).float() for t in state.values()]).to(dev)
        out = torch.empty_like(row)
        codes = torch.empty(n, dtype=torch.uint8, device=dev)
        keys = torch.empty(len(table), dtype=torch.int32, device=dev)
        work = torch.empty(lib.plato_agg_qsgd_encode_workspace(len(table), n), dtype=torch.uint8, device=dev)
        ptr = torch.tensor([row.data_ptr()], dtype=torch.int64, device=dev)
        print(f"ResNet-{depth}: n={n} entries={len(pieces)} row_MB={n * 4 / 1e6:.1f} level={args.level} reps={args.reps}")

        def encode_call():
            _lib.call("plato_agg_qsgd_encode", row.data_ptr(), n, table.ctypes.data, len(table), args.level, 7,
                      codes.data_ptr(), keys.data_ptr(), work.data_ptr(), sh)

        def mean_call():
            _lib.call("plato_agg_mean_rows", ptr.data_ptr(), None, 1, out.data_ptr(), None, n, 0, sh)

        calls = {"encode": encode_call, "mean_rows": mean_call}
        for fn in calls.values():
            fn()
        torch.cuda.synchronize()
        events = {name: [] for name in calls}
        for _ in range(args.reps):
            for name, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                events[name].append((e0, e1))
        torch.cuda.synchronize()
        times = {name: [e0.elapsed_time(e1) * 1e3 for e0, e1 in evs] for name, evs in events.items()}
        # the whole host call, wall clock (it ends with a blocking D2H copy)
        host.encode_state_dict(state, args.level, 7, dev)
        whole = []
        for _ in range(max(3, args.reps // 4)):
            t0 = time.perf_counter()
            wire = host.encode_state_dict(state, args.level, 7, dev)
            whole.append((time.perf_counter() - t0) * 1e6)
        times["encode_state_dict"] = whole
        med = {name: statistics.median(us) for name, us in times.items()}
        per_elem = {"encode": 9, "mean_rows": 8, "encode_state_dict": 9}
        for name, us in times.items():
            gbs = per_elem[name] * n / med[name] / 1e3
            print(f"  {name:18s} median {med[name]:10.1f} us   min {min(us):10.1f} us   max {max(us):10.1f} us   "
                  f"{med[name] / med['mean_rows']:8.2f} x mean_rows   {per_elem[name]} B/element   {gbs:8.1f} GB/s")
        # what the kernel left is what the host call returned
        got = codes.cpu().numpy()
        same = all(wire[name][10 + 2 * t.dim():] == got[b:e].tobytes() for (name, t), (b, e) in zip(state.items(), pieces))
        print(f"  the kernel's codes equal encode_state_dict's: {same}   wire bytes {sum(len(v) for v in wire.values())}")
        sys.stdout.flush()


if __name__ == "__main__":
    main()
