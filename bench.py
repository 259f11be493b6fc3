#!/usr/bin/env python3
"""Benchmark of the MI355X FedAvg aggregation engine (BASELINE.json metric).

Metric: aggregated GB/s (device-resident) of the fused FedAvg update over K
client model updates = algorithmic bytes / time, with algorithmic bytes
(K+2)·P_f32·4 + (K+2)·P_i64·8.

Workload (one "step" = one pass of the hot path over one batch):
  BASELINE config C2 — 128 synthetic client updates of CIFAR ResNet-18
  (11,183,562 fp32 + 20 int64 entries) aggregated into a new global model,
  inputs resident in HBM.  With --gpus N (one process per GPU, launched by
  torch.distributed.run) the ONE job is parameter-bucket sharded over the N
  GPUs (SURVEY.md §8(e), strong scaling): rank r aggregates bucket r of all
  128 clients, then an RCCL all-gather assembles the new model on every GPU.
  Both the kernel and the all-gather are inside the timed region; value =
  the job's algorithmic bytes / wall time per step.  (--scaling weak gives
  every rank its own model-sized job instead.)

A plain run sets up, warms up, times the steps and prints the result line, with
the roofline of the kernel from the HIP events of the timed steps.  ``--full``
adds the legs beside the headline (rank 0, N=1): the committed profile's
traffic, the host-inclusive and variant-server legs, and the reference's CPU op
sequence (oracle port) timed on this host on the same inputs, whose result is
also checked bit for bit; at N>1 the parity check against the one-GPU kernel
and the server's in-process multi-GPU leg.  ``--dump-outputs DIR`` writes the
last timed step's results as ``.npy`` files.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
ROOT = os.path.dirname(os.path.abspath(__file__))


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--config", default="C2", choices=sorted(CONFIGS),
                   help="BASELINE.json configuration (C2 = the headline metric's workload)")
    p.add_argument("--clients", type=int, default=None, help="override K")
    p.add_argument("--codec", default="native", choices=["native", "bf16"],
                   help="payload codec: bf16 = model_quantize'd payloads, kept bf16 in HBM")
    p.add_argument("--variant", type=int, default=None, help="kernel variant (tuning)")
    p.add_argument("--sweep", action="store_true", help="time every kernel variant, interleaved")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--full", action="store_true",
                   help="after the timed steps also run everything beside the headline figure: the committed "
                        "profile's roofline fields, the host-inclusive, variant-reduction and CPU-baseline legs "
                        "(N = 1), the parity check and the engine-devices leg (N > 1); the --no-* options trim it")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps write what the last step computed (the new model's fp32 arena and "
                        "its int64 entries' results) as DIR/<name>.npy, float32, at most 64 MB in all (a fixed "
                        "seeded sample of a larger array); the same arguments give the same inputs in every run")
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--no-host-inclusive", action="store_true")
    p.add_argument("--cpu-reps", type=int, default=3)
    p.add_argument("--streaming", action="store_true",
                   help="also time arrival staging and the trigger-to-result latency (C4, examples/async)")
    p.add_argument("--scaling", default="strong", choices=["strong", "weak"],
                   help="strong: one job bucket-sharded over the ranks (+ all-gather); weak: a job per rank")
    p.add_argument("--pieces", type=int, default=None,
                   help="strong scaling, N>1: each rank's bucket in this many pieces, the all-gather of "
                        "piece p running on RCCL's stream while the kernels of the later pieces run "
                        "(default: PIECES_BY_WORLD, chosen from the one-GPU anchor, DESIGN.md §6)")
    p.add_argument("--anchor", action="store_true",
                   help="one process, one GPU, no collective: time one rank's piece kernels for N = 1, 2, 4, 8 "
                        "(C2 and C3) and the grid-tail shapes of the headline kernel; JSON lines, not the metric")
    p.add_argument("--client-split", action="store_true",
                   help="with --engine-devices N: also time the client-split round (FedAdp / Port over N devices): "
                        "the assembly of each device's client arenas, and FedAdp's dots")
    p.add_argument("--probe-launch", action="store_true",
                   help="launcher check without a GPU: every rank joins a gloo group, rank 0 prints one JSON line")
    p.add_argument("--no-variants", action="store_true",
                   help="skip the variant servers' reductions leg (SURVEY.md §8(f), N=1 only)")
    p.add_argument("--variant-reps", type=int, default=10)
    p.add_argument("--variants-first", action="store_true",
                   help="N=1: run the variant reductions leg right after the headline's timed region, before the "
                        "host-inclusive leg (which leaves another K-client slab allocated)")
    p.add_argument("--dist-timeout", type=float, default=180.0,
                   help="N > 1: seconds any collective (and the rendezvous) may wait before the rank fails "
                        "naming it; also the per-rank stall watchdog (+60 s)")
    p.add_argument("--launch-timeout", type=float, default=900.0,
                   help="N > 1 self-launch: wall-clock seconds for the whole rank tree; on expiry its process "
                        "group is killed and each rank's last phase is printed (exit 124)")
    p.add_argument("--no-engine-devices-leg", action="store_true",
                   help="N > 1 strong scaling: skip the server's in-process multi-GPU leg (MultiDeviceEngine over "
                        "the N GPUs, run by rank 0 in a child process after the ranks have finished)")
    p.add_argument("--probe-stall-rank", type=int, default=-1,
                   help="with --probe-launch: this rank sleeps instead of joining the collective (timeout tests)")
    p.add_argument("--parity", action="store_true",
                   help="with --engine-devices: check the host result and every GPU's gathered copy bit for bit "
                        "against the one-GPU engine on the same payloads")
    p.add_argument("--engine-devices", type=int, default=0,
                   help="single-process multi-GPU engine (plato_amd.multi) over this many devices: host-inclusive "
                        "and device-resident timings of the server's own path (repeats cuda:0 on a 1-GPU box)")
    return p.parse_args()


# name -> (model, K).  At --gpus N the job is bucket-sharded over the N ranks
# (strong scaling, the default) or replicated per rank (--scaling weak).
CONFIGS = {
    "C1": ("lenet5", 10),
    "C2": ("resnet18", 128),
    "C3": ("resnet50_200", 1024),
    "C4": ("resnet18", 256),
    "C5": ("vit_large", 32),
    "C5-gpt2": ("gpt2_medium", 32),
}
BASELINE_METRIC = "aggregated GB/s (device-resident), K-client ResNet-18 FedAvg at 1/2/4/8 GPUs"


def model_spec(name):
    from plato_amd import workloads

    return {
        "resnet18": lambda: workloads.resnet(18, 10),
        "resnet50_200": lambda: workloads.resnet(50, 200),
        "lenet5": lambda: workloads.lenet5(10),
        "vit_large": lambda: workloads.vit_large(),
        "gpt2_medium": lambda: workloads.gpt2_medium(),
    }[name]()


def self_launch(n: int, argv: list[str], limit_s: float) -> int:
    """``bench.py --gpus N`` started plainly: run it under torch.distributed.run, one rank per GPU.

    Called before anything touches the GPU (no torch.cuda call in this process): the N ranks are
    a child process tree in its own process group (never an exec of this one).  Rank 0's JSON line
    is forwarded to this process's stdout; everything else the ranks write goes to stderr, so the
    result line stays the only stdout line.  The tree gets ``limit_s`` seconds of wall clock: on
    expiry its process group is killed and the last phase each rank announced (``[bench] rank r:
    ...`` lines, which name the collective a rank entered) is printed; the exit code is then 124.
    Returns the child's exit code otherwise.
    """
    import collections
    import signal
    import socket
    import subprocess
    import threading

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr=127.0.0.1", f"--master-port={port}", os.path.abspath(__file__), *argv]
    env = dict(os.environ, TORCH_NCCL_ASYNC_ERROR_HANDLING="1")
    progress(f"--gpus {n} without a torch.distributed world: launching {n} ranks (port {port}, "
             f"limit {limit_s:.0f} s)")
    child = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, bufsize=1, env=env,
                             start_new_session=True)
    tail = collections.deque(maxlen=40)
    phases: dict = {}

    def pump_out():
        for line in child.stdout:
            if line.startswith("{"):
                sys.stdout.write(line)
                sys.stdout.flush()
            else:
                sys.stderr.write(line)

    def pump_err():
        for line in child.stderr:
            sys.stderr.write(line)
            tail.append(line.rstrip("\n"))
            marker = line.find("[bench] rank ")
            if marker >= 0:
                head = line[marker + len("[bench] rank "):]
                r = head.split(":", 1)[0].strip()
                if r.isdigit():
                    phases[int(r)] = head.split(":", 1)[1].strip() if ":" in head else head.strip()

    readers = [threading.Thread(target=f, daemon=True) for f in (pump_out, pump_err)]
    for t in readers:
        t.start()
    try:
        code = child.wait(timeout=limit_s)
    except subprocess.TimeoutExpired:
        for sig, grace in ((signal.SIGTERM, 10), (signal.SIGKILL, 10)):
            try:
                os.killpg(child.pid, sig)
            except ProcessLookupError:
                break
            try:
                child.wait(timeout=grace)
                break
            except subprocess.TimeoutExpired:
                continue
        for t in readers:
            t.join(timeout=5)
        print(f"[bench] TIMEOUT: the {n}-rank tree exceeded --launch-timeout {limit_s:.0f} s and was killed; "
              "last phase per rank:", file=sys.stderr, flush=True)
        for r in range(n):
            print(f"[bench]   rank {r}: {phases.get(r, 'no phase reported (still starting)')}", file=sys.stderr,
                  flush=True)
        print("[bench] last stderr lines of the tree:", file=sys.stderr, flush=True)
        for line in list(tail)[-15:]:
            print(f"[bench]   | {line}", file=sys.stderr, flush=True)
        return 124
    for t in readers:
        t.join(timeout=5)
    return code


_WATCHDOG_S = None


def collective(rank: int, name: str, fn, *a, **kw):
    """Run one collective of the N > 1 path: announce it (the self-launcher's per-rank phase) and turn a
    failure (a peer gone, the --dist-timeout expired) into an error that names this rank and collective.
    Re-arms the per-rank watchdog: it fires only when one phase outlasts it."""
    progress(f"rank {rank}: {name}")
    if _WATCHDOG_S is not None:
        import faulthandler

        faulthandler.dump_traceback_later(_WATCHDOG_S, exit=True)
    try:
        return fn(*a, **kw)
    except Exception as exc:  # torch.distributed raises RuntimeError / DistBackendError subclasses
        raise RuntimeError(f"rank {rank}: collective {name!r} failed: {exc}") from exc


def arm_watchdog(args, world: int) -> None:
    """N > 1: a rank stalled between two collectives (a kernel or a host wait that never returns) dumps every
    thread's Python stack to stderr and exits non-zero once --dist-timeout + 60 s pass without a new phase
    (faulthandler, re-armed by every collective; no exec)."""
    global _WATCHDOG_S
    if world > 1:
        import faulthandler

        _WATCHDOG_S = args.dist_timeout + 60.0
        faulthandler.dump_traceback_later(_WATCHDOG_S, exit=True)


def disarm_watchdog() -> None:
    global _WATCHDOG_S
    if _WATCHDOG_S is not None:
        import faulthandler

        faulthandler.cancel_dump_traceback_later()
        _WATCHDOG_S = None


def probe_launch(args) -> None:
    """The launcher's plumbing on CPU: every rank joins a gloo group and sums its rank; rank 0 prints."""
    import torch.distributed as dist

    import datetime

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world > 1:
        progress(f"rank {rank}: init_process_group(gloo)")
        dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=args.dist_timeout))
    t = torch.tensor([float(rank)])
    if rank == args.probe_stall_rank:
        progress(f"rank {rank}: stalling before all_reduce (--probe-stall-rank)")
        time.sleep(3600)
    if world > 1:
        collective(rank, "all_reduce(rank_sum)", dist.all_reduce, t)
    if rank == 0:
        print(json.dumps({"probe": "launch", "n_gpus": world, "requested": args.gpus,
                          "rank_sum": float(t.item())}), flush=True)
    if world > 1:
        dist.destroy_process_group()


def dist_setup(args):
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("--gpus N>1 must be launched with torch.distributed.run (one process per GPU)")
    backend = os.environ.get("PLATO_BENCH_BACKEND", "nccl")
    ndev = torch.cuda.device_count()
    if local >= ndev:
        if backend != "gloo":
            raise SystemExit(f"rank {rank}: LOCAL_RANK {local} but only {ndev} GPU(s); one process per GPU "
                             "(set PLATO_BENCH_BACKEND=gloo to rehearse several ranks on one GPU)")
        local = local % ndev  # rehearsal only: ranks share a GPU
    torch.cuda.set_device(local)
    if world > 1:
        import datetime

        import torch.distributed as dist

        arm_watchdog(args, world)
        timeout = datetime.timedelta(seconds=args.dist_timeout)
        if backend == "nccl":  # RCCL over xGMI
            collective(rank, "init_process_group(nccl)", dist.init_process_group, "nccl",
                       device_id=torch.device("cuda", local), timeout=timeout)
        else:
            collective(rank, f"init_process_group({backend})", dist.init_process_group, backend, timeout=timeout)
    return world, rank, local


def barrier(world, what: str = "barrier"):
    if world > 1:
        import torch.distributed as dist

        collective(dist.get_rank(), what, dist.barrier)


def max_over_ranks(value: float, world: int, what: str = "max over ranks") -> float:
    if world == 1:
        return value
    import torch.distributed as dist

    dev = "cpu" if dist.get_backend() == "gloo" else "cuda"
    t = torch.tensor([value], dtype=torch.float64, device=dev)
    collective(dist.get_rank(), f"all_reduce(MAX, {what})", dist.all_reduce, t, op=dist.ReduceOp.MAX)
    return float(t.item())


def kernel_signature(variant: int) -> str:
    """The mangled-name fragment rocprofv3 reports for the fused kernel variant this bench launches."""
    import ctypes

    from plato_amd import _lib

    bs, v, u, fl = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.tune_call("plato_agg_tune_describe", variant, ctypes.byref(bs), ctypes.byref(v), ctypes.byref(u), ctypes.byref(fl))
    f = fl.value
    b = lambda x: "true" if x else "false"  # noqa: E731
    return (f"fedavg_kernel<(anonymous namespace)::Cfg<{bs.value}, {v.value}, {u.value}, {b(f & 1)}, {b(f & 2)}, "
            f"{b(f & 4)}, {b(f & 8)}, {(f >> 4) & 255}, {b(f & (1 << 12))}, {b(f & (1 << 13))}>, true, false>")


def source_stamp() -> str:
    """sha256[:16] of the hot kernel's source: a profile summary records it, so a stale one shows."""
    import hashlib

    with open(os.path.join(ROOT, "plato_amd", "csrc", "fedavg_agg.hip"), "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


def pmc_traffic(alg_bytes: int, kernel: str):
    """The committed rocprofv3 summary of this workload and kernel (PMC traffic + kernel-trace timing).

    PMC counters cannot be read from inside a timed run; scripts/profile.sh
    runs this bench once unprofiled and then under rocprofv3 (kernel trace,
    FETCH_SIZE and WRITE_SIZE in their own passes) in the same GPU lease, and
    scripts/summarize_profile.py writes profiles/<tag>_summary.json with the
    unprofiled run's ms_per_step / kernel_ms beside the profile's durations.
    A summary counts only if it profiled the same algorithmic bytes AND the
    same kernel instantiation; among those the newest tag wins, and one built
    from the current kernel source is preferred.
    """
    import glob

    stamp = source_stamp()
    found = []
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_summary.json"))):
        try:
            with open(path) as f:
                summ = json.load(f)
        except (OSError, ValueError):
            continue
        if summ.get("algorithmic_bytes") == alg_bytes and kernel in summ.get("kernel", ""):
            found.append((summ.get("source_sha16") == stamp, path, summ))
    if not found:
        return None
    current, path, summ = max(found, key=lambda x: (x[0], x[1]))
    summ = dict(summ, path=os.path.relpath(path, ROOT), current_source=current)
    return summ


def profile_roofline(summ, alg_bytes: int, kernel_ms: float, ms_per_step: float):
    """Roofline fields taken from the committed profile, and how they compare with this run."""
    if summ is None:
        return {"traffic": None, "traffic_source": None}
    # primary: the profile's timed-region dispatches (what ms_per_step covers); older summaries carried the
    # rocprof stats average over every call (warm-up included) as avg_duration_ms
    timed = summ.get("timed_avg_ms") or summ.get("avg_duration_ms")
    every = summ.get("rocprof_stats_avg_ms") or summ.get("avg_duration_ms")
    out = {
        "traffic": summ["pmc"]["hbm_bytes"],
        "traffic_source": summ["path"],
        "traffic_source_current": summ["current_source"],
        "traffic_profile_avg_ms": timed,
        "traffic_profile_all_calls_avg_ms": every,
        # the profile's own roofline: algorithmic bytes / the rocprofv3 kernel-trace duration
        "frac_profile": round(alg_bytes / (timed * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if timed else None,
        "frac_profile_all_calls": round(alg_bytes / (every * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if every else None,
        "profile_over_this_run_kernel_ms": round(timed / kernel_ms, 4) if timed else None,
        # a profile slower than this run's whole step was measured on another box / clock
        "profile_avg_exceeds_ms_per_step": bool(timed and timed > ms_per_step),
        "profile_lease_bench": summ.get("bench_same_lease"),
    }
    return out


def cpus_available() -> int:
    """CPUs this process can actually use: its affinity set, capped by a cgroup CPU quota.

    On a shared GPU box nproc shows every CPU of the machine while the job's
    cgroup grants a share of them; oversubscribing that share only slows the
    baseline down.
    """
    try:
        n = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        n = os.cpu_count() or 1
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()[:2]
        if quota != "max":
            n = min(n, max(1, -(-int(quota) // int(period))))
    except (OSError, ValueError):
        pass
    return n


def progress(msg: str) -> None:
    """A line on stderr per phase (the JSON result line stays the only stdout line)."""
    print(f"[bench] {msg}", file=sys.stderr, flush=True)


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args.gpus, sys.argv[1:], args.launch_timeout))
    if args.probe_launch:
        return probe_launch(args)
    if args.anchor:
        return anchor_bench(args)
    world, rank, local = dist_setup(args)
    dev = torch.device("cuda", local)

    from plato_amd import _lib
    from plato_amd.arena import ArenaLayout
    from plato_amd.engine import ClientSlab, DeviceArena, FedAvgEngine
    from plato_amd.synthetic import fill_baseline, fill_clients

    if args.engine_devices:
        return engine_devices_bench(args)
    model, k_default = CONFIGS[args.config]
    scaling = args.scaling
    k = args.clients or k_default
    full_layout = ArenaLayout.from_shapes(model_spec(model))
    plan = xchg = None
    pieces = 1
    if scaling == "strong" and world > 1:
        # one model, parameter-bucket sharded and cut into `pieces` round-robin pieces: piece
        # j = p * world + r belongs to rank r, so the p-th pieces of all ranks are contiguous in
        # the model and one all-gather per p assembles them in place
        from plato_amd.distributed import PiecePlan

        pieces = max(1, args.pieces or pieces_for(args.config, world))
        progress(f"rank {rank}: {pieces} pieces per rank "
                 + ("(--pieces)" if args.pieces else "(PIECES_BY_WORLD, from the one-GPU anchor)"))
        plan = PiecePlan.for_layout(full_layout, world, pieces)
        xchg = plan.exchange(full_layout.n_i64)
        piece_n = [plan.piece_elements(rank, p) for p in range(pieces)]
        n_i64_loc = full_layout.n_i64 if rank == 0 else 0
        layout = ArenaLayout([], pieces * plan.length, n_i64_loc)
        job_bytes = full_layout.algorithmic_bytes(k)
    else:
        layout = full_layout
        job_bytes = world * full_layout.algorithmic_bytes(k)
    # ONE job: every rank uses the same seed, so its pieces are slices of the one global baseline and
    # client set (and every rank the same num_samples); weak scaling gives each rank the same job again
    seed = args.seed
    engine = FedAvgEngine(dev, variant=args.variant)

    base = DeviceArena(layout, dev)
    slab = ClientSlab(layout, k, dev)
    if plan is not None:
        from plato_amd.synthetic import fill_slices

        slices = [(p * plan.length, plan.piece_range(rank, p)[0], piece_n[p]) for p in range(pieces) if piece_n[p]]
        fill_slices(base, slab, slices, n_i64_loc, seed, k)
    else:
        fill_baseline(base, seed)
        fill_clients(slab, base, seed, k)
    if args.codec == "bf16":  # model_quantize'd payloads (every entry .to(bfloat16))
        slab16 = ClientSlab(layout, k, dev, codec="bf16")
        slab16.f32.copy_(slab.f32.to(torch.bfloat16))
        slab16.i64.copy_(slab.i64.to(torch.bfloat16))
        del slab
        torch.cuda.empty_cache()
        slab = slab16

    from plato_amd import synthetic
    from plato_amd import weights as W
    from plato_amd.engine import fp32_weights

    ns = synthetic.num_samples(k, seed)
    if args.config == "C4":  # async staleness-weighted (Port, examples/async/port/port_cifar10.yml)
        weights = W.port(ns, synthetic.staleness(k, seed), similarity_weight=1, staleness_weight=3)
    else:
        weights = W.fedavg(ns)
    w = torch.from_numpy(fp32_weights(weights)).to(dev)
    pf, pi = slab.row_pointers(range(k))
    tf = torch.from_numpy(pf).to(dev)
    ti = torch.from_numpy(pi).to(dev)
    if plan is not None:
        # send buffer: [piece 0 | int64 results (meaningful on rank 0) | piece 1 | ... ]; the
        # all-gather of piece p lands in gathered[goff[p]:], ranks in model order (PieceExchange)
        L = plan.length
        send = torch.zeros(xchg.send_numel, dtype=torch.float32, device=dev)
        soff = xchg.soff
        gathered = torch.empty(xchg.gathered_numel, dtype=torch.float32, device=dev)
        out_i = send[xchg.int64_offset(): xchg.int64_offset() + xchg.ipad]
        # per piece: client-row pointers offset to the piece (rows are pieces * L long)
        piece_tf = [torch.from_numpy(pf + p * L * 4).to(dev) for p in range(pieces)]
        piece_lay = [ArenaLayout([], piece_n[p], layout.n_i64 if p == 0 else 0) for p in range(pieces)]
        out_f = send  # (unused for N>1 beyond the slices below)
    else:
        out_f = torch.empty(layout.row_f32, dtype=torch.float32, device=dev)
        out_i = torch.empty(layout.row_i64, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev)
    torch.cuda.synchronize(dev)

    if args.codec == "bf16" and plan is not None:
        raise SystemExit("--codec bf16 is timed per GPU only (--scaling weak) for --gpus N>1")

    def kernel(variant=None):
        if args.codec == "bf16":
            v = (args.variant or 0) if variant is None else variant
            _lib.tune_call("plato_agg_tune_fedavg_bf16", v, tf.data_ptr(), ti.data_ptr(), w.data_ptr(), None, k,
                      base.f32.data_ptr(), base.i64.data_ptr(), out_f.data_ptr(), out_i.data_ptr(),
                      layout.n_f32, layout.n_i64, stream.cuda_stream)
            return
        engine.variant = args.variant if variant is None else variant
        if plan is None:
            engine.launch_fedavg(layout, tf, ti, w, None, k, base.f32, base.i64, out_f, out_i, stream)
            return
        for p in range(pieces):
            kernel_piece(p)
            start_gather(p)

    rehearsal = world > 1 and os.environ.get("PLATO_BENCH_BACKEND", "nccl") == "gloo"
    pending = []

    def kernel_piece(p):
        lay = piece_lay[p]
        if lay.n_f32 or lay.n_i64:
            engine.launch_fedavg(lay, piece_tf[p], ti, w, None, k, base.f32[p * L:], base.i64,
                                 send[soff[p]:], out_i, stream)

    def start_gather(p):
        """All-gather of piece p: on RCCL's own stream, ordered after the kernels enqueued so far
        and concurrent with the later pieces' kernels (async_op; waited for in assemble())."""
        import torch.distributed as dist

        src = xchg.send_slice(send, p)
        dst = xchg.gather_slice(gathered, p)
        if rehearsal:  # gloo moves host tensors (ranks sharing one GPU)
            host = torch.empty(dst.numel(), dtype=torch.float32)
            dist.all_gather_into_tensor(host, src.cpu())
            dst.copy_(host)
        else:  # RCCL over xGMI
            pending.append(dist.all_gather_into_tensor(dst, src, async_op=True))

    def assemble():
        while pending:
            pending.pop(0).wait()  # the launch stream waits for RCCL's stream

    def step(variant=None):
        kernel(variant)
        assemble()

    alg_bytes = (layout.algorithmic_bytes(k) if plan is None
                 else sum(lay.algorithmic_bytes(k) for lay in piece_lay))  # this rank's pieces, no padding
    if args.codec == "bf16":  # K bf16 client arenas + fp32 baseline and result
        alg_bytes = k * 2 * (layout.n_f32 + layout.n_i64) + 2 * (layout.n_f32 * 4 + layout.n_i64 * 8)
        job_bytes = (alg_bytes * world if plan is None else
                     k * 2 * (full_layout.n_f32 + full_layout.n_i64) + 2 * (full_layout.n_f32 * 4 + full_layout.n_i64 * 8))

    if args.sweep and args.codec == "bf16":
        nv = _lib.tune().plato_agg_tune_num_bf16_variants()
        times = {v: [] for v in range(nv)}
        for v in range(nv):
            kernel(v)
        torch.cuda.synchronize(dev)
        for _ in range(5):
            for v in range(nv):
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(args.steps):
                    kernel(v)
                e1.record(stream)
                e1.synchronize()
                times[v].append(e0.elapsed_time(e1) / args.steps)
        if rank == 0:
            for v in range(nv):
                med = statistics.median(times[v])
                print(json.dumps({"bf16_variant": v, "ms_median": med,
                                  "GBps": alg_bytes / (med * 1e-3) / 1e9}), flush=True)
        return

    if args.sweep:
        nv = _lib.tune().plato_agg_tune_num_variants()
        times = {v: [] for v in range(nv)}
        for v in range(nv):
            for _ in range(3):
                kernel(v)
        torch.cuda.synchronize(dev)
        for _ in range(5):
            for v in range(nv):
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(args.steps):
                    kernel(v)
                e1.record(stream)
                e1.synchronize()
                times[v].append(e0.elapsed_time(e1) / args.steps)
        # measured streaming ceilings over the same byte count (5.8 GB for C2)
        n_probe = (alg_bytes // 4) // 8 * 8
        src = torch.empty(n_probe, dtype=torch.float32, device=dev)
        src.fill_(1.0)
        dst = torch.empty(n_probe // 2 + 64, dtype=torch.float32, device=dev)
        probes = {}
        for mode, name, nbytes in ((1, "read", n_probe * 4), (0, "copy", (n_probe // 2) * 8)):
            for blocks in (1024, 2048, 4096, 8192):
                n_el = n_probe if mode == 1 else n_probe // 2
                _lib.tune_call("plato_agg_tune_stream", mode, src.data_ptr(), dst.data_ptr(), n_el, blocks,
                          stream.cuda_stream)
                torch.cuda.synchronize(dev)
                ts = []
                for _ in range(5):
                    e0 = torch.cuda.Event(enable_timing=True)
                    e1 = torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    _lib.tune_call("plato_agg_tune_stream", mode, src.data_ptr(), dst.data_ptr(), n_el, blocks,
                              stream.cuda_stream)
                    e1.record(stream)
                    e1.synchronize()
                    ts.append(e0.elapsed_time(e1))
                probes[f"{name}_b{blocks}"] = nbytes / (statistics.median(ts) * 1e-3) / 1e9
        del src, dst
        if rank == 0:
            import ctypes

            print(json.dumps({"ceilings_GBps": {k: round(v, 1) for k, v in probes.items()}}), flush=True)

            for v in range(nv):
                bs, a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
                _lib.tune().plato_agg_tune_describe(v, ctypes.byref(bs), ctypes.byref(a), ctypes.byref(b),
                                                   ctypes.byref(c))
                med = statistics.median(times[v])
                print(json.dumps({"variant": v, "B": bs.value, "V": a.value, "U": b.value,
                                  "ntl": c.value & 1, "nts": (c.value >> 1) & 1, "pipe": (c.value >> 2) & 1,
                                  "buf": (c.value >> 3) & 1, "persist": (c.value >> 4) & 255, "xcd": (c.value >> 12) & 1,
                                  "ms_median": med, "ms_min": min(times[v]),
                                  "GBps": alg_bytes / (med * 1e-3) / 1e9}), flush=True)
        return

    progress(f"rank {rank}: inputs ready, {args.warmup} warmup + {args.steps} timed steps")
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize(dev)
    barrier(world)
    torch.cuda.synchronize(dev)
    # HIP events on the launch stream.  N = 1: one event before the first step and one after the last,
    # so the kernel time is the span over the K back-to-back launches divided by K (launch gaps
    # included); each event recorded between two launches costs the stream ~3-4 us
    # (profiles/r05c_anchor.log "launch_gaps": 0.9064 ms per launch with none, 0.9097 with one, 0.9182
    # with the three per step of rounds 1-4).  N > 1: events around the kernels and around the
    # assembly, which are timed apart.
    if plan is None:
        bounds = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        t0 = time.perf_counter()
        bounds[0].record(stream)
        for i in range(args.steps):
            kernel()
            assemble()
        bounds[1].record(stream)
    else:
        marks = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.steps)]
        t0 = time.perf_counter()
        for m in marks:
            m[0].record(stream)
            kernel()
            m[1].record(stream)
            assemble()
            m[2].record(stream)
    torch.cuda.synchronize(dev)
    barrier(world)
    torch.cuda.synchronize(dev)
    t1 = time.perf_counter()
    wall = max_over_ranks(t1 - t0, world)
    if plan is None:
        kernel_ms = bounds[0].elapsed_time(bounds[1]) / args.steps
        assembly_ms = 0.0
    else:
        kernel_ms = statistics.fmean(m[0].elapsed_time(m[1]) for m in marks)
        assembly_ms = statistics.fmean(m[1].elapsed_time(m[2]) for m in marks)
    kernel_ms_max = max_over_ranks(kernel_ms, world)
    assembly_ms_max = max_over_ranks(assembly_ms, world)

    value_gbs = job_bytes * args.steps / wall / 1e9
    variant = args.variant if args.variant is not None else 0
    if args.dump_outputs:
        # what a caller of the timed path holds after the last step: the new model (N > 1: as gathered)
        got_f, got_i = (out_f[: layout.n_f32], out_i[: layout.n_i64]) if plan is None else xchg.assemble(gathered)
        if rank == 0:
            dump_outputs(args.dump_outputs, {"model_f32": got_f, "model_i64_entries": got_i})
        del got_f, got_i
    summ = pmc_traffic(alg_bytes, kernel_signature(variant)) if args.full and args.codec == "native" else None
    achieved = alg_bytes / (kernel_ms_max * 1e-3) / 1e9
    prof = profile_roofline(summ, alg_bytes, kernel_ms_max, wall / args.steps * 1e3)

    result = {
        "metric": BASELINE_METRIC,
        "value": round(value_gbs, 2),
        "unit": "GB/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(wall / args.steps * 1e3, 4),
        "higher_is_better": True,
        "scaling": scaling,
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic (counter-based generator, SURVEY.md §8(d) C2 distributions)",
        "config": {
            "workload": f"{args.config}: {k} x {model} client updates, fused FedAvg "
                        "(deltas -> weighted sum -> update), inputs resident in HBM; "
                        + ("each rank aggregates its own model-sized job" if scaling == "weak" and world > 1
                           else f"one job bucket-sharded over {world} GPU(s)"
                           + (f", {pieces} pieces per rank, RCCL all-gather of each piece overlapping the "
                              "later pieces' kernels, all inside the timed region" if world > 1 else "")),
            "clients": k,
            "params_f32_per_gpu": layout.n_f32,
            "params_i64_per_gpu": layout.n_i64,
            "algorithmic_bytes_per_step_per_gpu": alg_bytes,
            "algorithmic_bytes_per_step_job": job_bytes,
            "parallelism": f"bucket{world}",
            "pieces_per_rank": pieces,
            "kernel_variant": variant,
            "payload_codec": args.codec,
            "kernel_ms_max_over_ranks": round(kernel_ms_max, 4),
            "assembly_ms_max_over_ranks": round(assembly_ms_max, 4),
        },
        "roofline": {
            "bound": "hbm",
            "achieved": round(achieved, 1),
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 4),
            "traffic": prof["traffic"],
            "traffic_unit": "bytes/launch (HBM, rocprofv3 PMC)",
            **{k2: v2 for k2, v2 in prof.items() if k2 != "traffic"},
            "kernel_ms": round(kernel_ms, 4),
            "kernel_ms_max_over_ranks": round(kernel_ms_max, 4),
            "kernel_source_sha16": source_stamp(),
        },
    }

    if args.codec != "native" or not args.full:
        args.no_host_inclusive = args.no_cpu_baseline = args.no_variants = args.no_engine_devices_leg = True
    run_variants = rank == 0 and world == 1 and not args.no_variants and args.config == "C2" and args.codec == "native"
    if run_variants and args.variants_first:
        progress("variant reductions leg")
        result["variants"] = variant_legs(dev, k, args.variant_reps)
        run_variants = False
    if rank == 0 and world == 1 and not args.no_host_inclusive:
        progress("host-inclusive leg")
        result["host_inclusive"] = host_inclusive(engine, layout, base, slab, k, weights, dev)

    if rank == 0 and world == 1 and args.streaming:
        result["streaming"] = streaming(engine, layout, base, slab, k, weights, dev)

    if run_variants:
        progress("variant reductions leg")
        result["variants"] = variant_legs(dev, k, args.variant_reps)

    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        progress("cpu baseline leg")
        result["cpu_baseline"] = cpu_baseline(layout, base, slab, k, weights, out_f, out_i, args.cpu_reps,
                                              args.config)
        result["parity"] = result["cpu_baseline"].pop("parity")

    exit_code = 0
    if plan is not None and args.full:
        # outside the timed region: the model every rank gathered in the last step, in model order,
        # must be the one-GPU fused kernel's result on the same global job (rank 0 recomputes it), bit
        # for bit, and every rank must hold the same bits
        torch.cuda.synchronize(dev)
        got_f, got_i = xchg.assemble(gathered)
        agree = ranks_agree(bits_digest(got_f, got_i), world)
        if rank == 0:
            progress(f"rank {rank}: parity check against the one-GPU kernel on the same job")
            par = check_against_one_gpu(engine, full_layout, k, seed, w, got_f, got_i, dev, stream)
            par["ranks_hold_identical_models"] = agree
            if not agree:
                par["parity"] = "MISMATCH: ranks gathered different models"
            result["parity"] = par.pop("parity")
            result["parity_detail"] = par
            if not result["parity"].startswith("bit-exact"):
                exit_code = 3
        del got_f, got_i
        barrier(world, "barrier after the parity check")
    if world > 1:
        import torch.distributed as dist

        progress(f"rank {rank}: destroy_process_group")
        dist.destroy_process_group()
        disarm_watchdog()  # what follows is bounded on its own (the engine-devices leg's limit)
    if rank == 0 and plan is not None and not args.no_engine_devices_leg and args.codec == "native":
        # the server's own multi-GPU path (one process driving the N GPUs: MultiDeviceEngine, RCCL
        # communicator from ncclCommInitAll), in a child process once the ranks are done
        del slab, base, send, gathered
        torch.cuda.empty_cache()
        result["engine_devices"] = engine_devices_child(args, world)
        if str(result["engine_devices"].get("parity", "")).startswith("MISMATCH"):
            exit_code = 3
    if rank == 0:
        print(json.dumps(result), flush=True)
    if exit_code:
        sys.exit(exit_code)


DUMP_LIMIT_BYTES = 64 * 10**6


def dump_outputs(path: str, arrays: dict) -> None:
    """Write each result array as ``path/<name>.npy`` (float32), at most DUMP_LIMIT_BYTES in all.

    Arrays that fit are written whole.  Otherwise each is cut to its share of the limit: a sorted
    sample of positions drawn by a generator seeded with the array's length alone, so two runs (or
    two builds) with the same arguments write the same positions.
    """
    os.makedirs(path, exist_ok=True)
    total = sum(t.numel() * 4 for t in arrays.values())
    budget = DUMP_LIMIT_BYTES - 4096 * len(arrays)  # the .npy headers count too
    for name, t in arrays.items():
        t = t.reshape(-1).to(torch.float32)
        if total > budget:
            keep = max(1, int(budget / total * t.numel()) - 1)
            if keep < t.numel():
                idx = np.sort(np.random.default_rng(t.numel()).integers(0, t.numel(), size=keep))
                t = t[torch.from_numpy(idx).to(t.device)]
        np.save(os.path.join(path, f"{name}.npy"), t.cpu().numpy())


def bits_digest(f: torch.Tensor, i: torch.Tensor) -> list[int]:
    """Two order-sensitive int64 checksums of the bit patterns of (fp32 arena, int64-entry results)."""
    out = []
    for t in (f, i):
        b = t.contiguous().view(torch.int32).to(torch.int64)
        pos = torch.arange(b.numel(), device=b.device, dtype=torch.int64) % 65521 + 1
        out.extend([int(b.sum()), int((b * pos).sum())])
    return out


def ranks_agree(digest: list[int], world: int) -> bool:
    """Every rank's digest equal (all_reduce MAX and MIN)."""
    if world == 1:
        return True
    import torch.distributed as dist

    dev = "cpu" if dist.get_backend() == "gloo" else "cuda"
    hi = torch.tensor(digest, dtype=torch.int64, device=dev)
    lo = hi.clone()
    rank = dist.get_rank()
    collective(rank, "all_reduce(MAX, model digest)", dist.all_reduce, hi, op=dist.ReduceOp.MAX)
    collective(rank, "all_reduce(MIN, model digest)", dist.all_reduce, lo, op=dist.ReduceOp.MIN)
    return bool(torch.equal(hi, lo))


def check_against_one_gpu(engine, full_layout, k: int, seed: int, w: torch.Tensor, got_f: torch.Tensor,
                          got_i: torch.Tensor, dev, stream, budget: int | None = None) -> dict:
    """The one-GPU fused kernel on the whole job (the same K clients of ``seed``), compared bit for bit.

    The job is regenerated on this GPU by the same counter generator, in windows of the fp32 arena
    sized to ``budget`` bytes of client + baseline + result (the whole C2 model in one window; C3's
    1,024 clients in a few): every element is the same sequential-K chain whatever the window, so
    each window's launch is the one-GPU result for its elements.  The int64 entries run with the
    first window.
    """
    from plato_amd.arena import ROW_ALIGN, ArenaLayout
    from plato_amd.engine import ClientSlab, DeviceArena
    from plato_amd.synthetic import fill_slices

    n_f, n_i = full_layout.n_f32, full_layout.n_i64
    if budget is None:
        free, _ = torch.cuda.mem_get_info(dev)
        budget = min(free // 3, 24 << 30)
    per_elem = (k + 2) * 4
    win = max(ROW_ALIGN, min(max(n_f, 1), budget // per_elem) // ROW_ALIGN * ROW_ALIGN)
    lay = ArenaLayout([], win, n_i)
    base = DeviceArena(lay, dev)
    slab = ClientSlab(lay, k, dev)
    out_f = torch.empty(lay.row_f32, dtype=torch.float32, device=dev)
    out_i = torch.empty(max(lay.row_i64, 1), dtype=torch.float32, device=dev)
    pf, pi = slab.row_pointers(range(k))
    tf, ti = torch.from_numpy(pf).to(dev), torch.from_numpy(pi).to(dev)

    def run_window(lo, n, ni):
        fill_slices(base, slab, [(0, lo, n)] if n > 0 else [], ni, seed, k, stream)
        engine.launch_fedavg(ArenaLayout([], n, ni), tf, ti, w, None, k, base.f32, base.i64, out_f, out_i, stream)
        return out_f[:n], out_i[:ni]

    res = compare_windows(n_f, n_i, win, run_window, got_f, got_i)
    torch.cuda.synchronize(dev)
    res["reference"] = ("plato_agg_fedavg_weights on rank 0's GPU over the whole job, regenerated by "
                        "plato_agg_fill_synth_*_at (same seed, same clients, same weights)")
    return res


def compare_windows(n_f: int, n_i: int, win: int, run_window, got_f: torch.Tensor, got_i: torch.Tensor) -> dict:
    """Compare the gathered model with ``run_window(lo, n, ni) -> (fp32 results, int64-entry results)`` over
    windows of ``win`` fp32 elements (the int64 entries with the first), bit for bit; the parity fields."""
    mism, first_bad, windows = 0, None, 0
    for lo in range(0, max(n_f, 1), win):
        n = max(0, min(win, n_f - lo))
        ni = n_i if lo == 0 else 0
        if n == 0 and not ni:
            break
        ref_f, ref_i = run_window(lo, n, ni)
        windows += 1
        if n:
            bad = (ref_f.view(torch.int32) != got_f[lo:lo + n].view(torch.int32)).nonzero()
            if bad.numel():
                mism += int(bad.numel())
                first_bad = first_bad if first_bad is not None else lo + int(bad[0])
        if ni:
            bad_i = (ref_i.view(torch.int32) != got_i[:ni].view(torch.int32)).nonzero()
            mism += int(bad_i.numel())
            if bad_i.numel() and first_bad is None:
                first_bad = f"int64 entry {int(bad_i[0])}"
    return {"parity": "bit-exact vs 1-GPU kernel" if mism == 0 else "MISMATCH vs 1-GPU kernel",
            "elements_checked": n_f + n_i, "mismatched_elements": mism, "first_mismatch": first_bad,
            "windows": windows, "window_elements": win}


ENGINE_DEVICES_LIMIT_S = 300.0


def engine_devices_child(args, world: int) -> dict:
    """``bench.py --engine-devices N --parity`` as a child process (spawned, never exec'd); its JSON line.

    The child drives the N GPUs from one process (``MultiDeviceEngine``), as the Plato server does
    (plato/servers/base.py:323-327), and checks its results against the one-GPU engine.  Bounded by
    ``--launch-timeout``; a child that fails or times out is reported in the line, not retried.
    """
    import signal
    import subprocess

    env = {key: v for key, v in os.environ.items()
           if key not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "GROUP_RANK", "ROLE_RANK",
                          "ROLE_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "TORCHELASTIC_RUN_ID")}
    cmd = [sys.executable, os.path.abspath(__file__), "--engine-devices", str(world), "--config", args.config,
           "--steps", str(max(1, min(args.steps, 5))), "--warmup", "1", "--seed", str(args.seed), "--parity"]
    if args.clients:
        cmd += ["--clients", str(args.clients)]
    # bounded well inside the whole run's budget: the leg takes ~30-60 s (torch import, 128 host payloads,
    # a few rounds); a hang in its first in-process RCCL communicator must not cost the line
    limit = min(args.launch_timeout, ENGINE_DEVICES_LIMIT_S)
    progress(f"rank 0: engine-devices leg (limit {limit:.0f} s): {' '.join(cmd[1:])}")
    child = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, env=env, start_new_session=True)
    try:
        out, _ = child.communicate(timeout=limit)
    except subprocess.TimeoutExpired:
        os.killpg(child.pid, signal.SIGKILL)
        child.communicate()
        return {"status": "timeout", "limit_s": limit, "command": " ".join(cmd[1:])}
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    res = json.loads(lines[-1]) if lines else {}
    res["status"] = "ok" if child.returncode == 0 and lines else f"failed (exit {child.returncode})"
    if child.returncode:
        res["command"] = " ".join(cmd[1:])
    return res


# one dependent v_fmac_f32 step on MI355X: 4.04 shader cycles back to back from registers
# (scripts/micro/chain_b128.hip, profiles/r04_micro_chain_b128.log), the wave64 issue rate; the
# round-1 micro's 6.0 (scripts/micro/fma_chain.hip) included a taken loop branch every 16 steps
CHAIN_CYCLES = 4.0
# the same chain fed from LDS by ds_read_b128 (4 steps per read, one s_waitcnt per block), no other
# waves: 5.86-5.87 cycles per step (profiles/r04_micro_chain_b128.log).  Every chain kernel reads its
# operands this way: register-resident operands need another wave's data, global-memory operands ran
# 48-50 cycles per step (profiles/r05zf_micro_chain_global.log), so this is the rate the design can reach
LDS_FED_CHAIN_CYCLES = 5.86
CLOCK_HZ = 2.4e9


def variant_legs(dev, k: int, reps: int) -> dict:
    """The variant servers' whole-model reductions on the headline's inputs.

    K synthetic ResNet-18 clients in HBM, after the headline's timed region.  Per path: the
    HIP-event time of its kernels as the engine launches them (``AggregationRound.timings``), the
    wall time of the engine call (host sync and small D2H included), the kernels' algorithmic bytes
    and floor — the larger of those bytes at the HBM peak and, where the reference's float32 order
    is one serial fma chain per vector, that chain at CHAIN_CYCLES per step — and floor / kernel.
    FedAdp runs on arenas aligned to its flattened positions, as FedAdpServerMixin's rounds do.
    """
    from plato_amd import _lib
    from plato_amd.arena import F32, ArenaLayout
    from plato_amd.engine import ClientSlab, DeviceArena, FedAvgEngine, _ptr
    from plato_amd.synthetic import fill_baseline, fill_clients

    spec = model_spec("resnet18")
    slots = list(range(k))

    def make_round(align, deltas=False):
        lay = ArenaLayout.from_shapes(spec, align=align)
        base = DeviceArena(lay, dev)
        fill_baseline(base, 0)
        baseline = lay.unpack(base.f32.cpu(), base.i64.cpu())
        eng = FedAvgEngine(dev)
        eng.layout_align = align
        eng.delta_arenas = deltas
        rnd = eng.begin(baseline, k)
        rnd.put_baseline(baseline)
        torch.cuda.synchronize(dev)
        fill_clients(rnd.slab, eng._base, 0, k)
        for s in range(k):
            pf, pi = rnd.slab.row_pointers([s])
            rnd._pf[s], rnd._pi[s] = int(pf[0]), int(pi[0])
            rnd.staged[s] = True
        torch.cuda.synchronize(dev)
        rnd.delta_ms_per_client = None
        if deltas:  # what put_client does behind each client's H2D: the slot turned into x - b in place
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(rnd.stager.stream)
            for s in range(k):
                rnd._to_delta(s)
            e1.record(rnd.stager.stream)
            torch.cuda.synchronize(dev)
            rnd.delta_ms_per_client = e0.elapsed_time(e1) / k
        return lay, base, rnd

    def measure(fn, rnd, keys):
        fn()
        torch.cuda.synchronize(dev)
        walls, kernel = [], {key: [] for key in keys}
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            walls.append((time.perf_counter() - t0) * 1e3)
            for key in keys:
                kernel[key].append(rnd.timings[key + "_ms"])
        return statistics.median(walls), {key: statistics.median(v) for key, v in kernel.items()}

    def entry(kernel_ms, nbytes, chain_steps=0):
        hbm = nbytes / (HBM_PEAK_GBS * 1e9) * 1e3
        floor = max(hbm, chain_steps * CHAIN_CYCLES / CLOCK_HZ * 1e3)
        res = {"kernel_ms": round(kernel_ms, 4), "algorithmic_bytes": int(nbytes),
               "GBps": round(nbytes / (kernel_ms * 1e-3) / 1e9, 1), "serial_chain_steps": int(chain_steps),
               "floor_ms": round(floor, 4), "frac_of_floor": round(floor / kernel_ms, 4)}
        if chain_steps:  # the chain at the measured LDS-fed rate (LDS_FED_CHAIN_CYCLES), beside the 4-cycle floor
            lds = max(hbm, chain_steps * LDS_FED_CHAIN_CYCLES / CLOCK_HZ * 1e3)
            res.update(lds_fed_chain_floor_ms=round(lds, 4), frac_of_lds_fed_chain_floor=round(lds / kernel_ms, 4))
        return res

    out = {"clients": k, "model": "resnet18", "reps": reps,
           "note": "HIP events around each engine launch (AggregationRound.timings); outside the headline's timed "
                   "region; floor = max(algorithmic bytes at 8 TB/s, serial fma chain at 4 cycles/step, 2.4 GHz); "
                   "lds_fed_chain_floor = the same with the chain at its measured LDS-fed rate, 5.86 cycles/step"}
    lay, base, rnd = make_round(None)
    n_f, n_i = lay.n_f32_data, lay.n_i64
    model_bytes = n_f * 4 + n_i * 8
    n_flat = n_f + n_i
    longest = max(e.numel for e in lay.entries if e.region == F32)

    # FedAdp: global gradient (entrywise pass) + the fused gather/sdot kernel, aligned arenas holding each
    # client's delta (FedAdpServerMixin.arena_deltas: formed behind each client's H2D at staging)
    lay_a, _, rnd_a = make_round("fedadp", deltas=True)
    w1 = np.full((len(lay_a.entries), k), 1.0 / k)

    def fedadp():
        grads = rnd_a.launch_entrywise(w1, add_base=False, device=True)
        rnd_a.fedadp_dots(grads, slots, 0.01)

    wall, km = measure(fedadp, rnd_a, ["fedadp_dots"])
    out["fedadp"] = dict(entry(km["fedadp_dots"], k * model_bytes + 2 * n_flat * 4, n_flat // 64),
                         path_ms=round(wall, 3), kernel="plato_agg_fedadp_dots (prep + dots + finish), delta arenas",
                         staging_delta_ms_per_client=round(rnd_a.delta_ms_per_client, 4),
                         reference="examples/server_aggregation/fedadp/fedadp_server.py:91-99")
    del rnd_a
    torch.cuda.empty_cache()
    # the same kernel on weight arenas (the baseline streamed beside every client), for comparison
    _, _, rnd_w = make_round("fedadp")

    def fedadp_w():
        grads = rnd_w.launch_entrywise(w1, add_base=False, device=True)
        rnd_w.fedadp_dots(grads, slots, 0.01)

    wall, km = measure(fedadp_w, rnd_w, ["fedadp_dots"])
    out["fedadp_weight_arenas"] = dict(entry(km["fedadp_dots"], k * model_bytes + 3 * n_flat * 4, n_flat // 64),
                                       path_ms=round(wall, 3), kernel="plato_agg_fedadp_dots, weight arenas")
    del rnd_w
    torch.cuda.empty_cache()

    # Port: norms gathered from the arenas (8 torch-order chains per vector) + cosine sums
    prev = DeviceArena(lay, dev)
    fill_baseline(prev, 1)
    previous = lay.unpack(prev.f32.cpu(), prev.i64.cpu())
    del prev
    prev_arena = rnd.stage_reference(previous)
    wall, km = measure(lambda: rnd.model_similarities(prev_arena, slots), rnd, ["port_norms", "port_cosine"])
    out["port_norms"] = dict(entry(km["port_norms"], (k + 2) * model_bytes + (k + 1) * n_flat * 4, n_flat // 8),
                             path_ms=round(wall, 3), kernel="plato_agg_port_norms",
                             reference="examples/async/port/port_server.py:38-50")
    out["port_cosine"] = dict(entry(km["port_cosine"], (k + 1) * n_flat * 4), kernel="plato_agg_scale_by_norm + "
                              "plato_agg_torch_cosine_sum_scaled", reference="examples/async/port/port_server.py:50")
    torch.cuda.empty_cache()

    # FedAtt: per-(entry, client) torch norms; Polaris: numpy pairwise squared sums per entry
    wall, km = measure(lambda: rnd.entry_norms(slots), rnd, ["entry_norms"])
    out["fedatt_norms"] = dict(entry(km["entry_norms"], (k + 1) * n_f * 4, longest // 8), path_ms=round(wall, 3),
                               kernel="plato_agg_entry_norms_f32",
                               reference="examples/server_aggregation/fedatt/fedatt_algorithm.py:34-39")
    wall_w, km_w = measure(lambda: rnd.np_sumsq(slots), rnd, ["np_sumsq"])
    # Polaris' rounds stage deltas (PolarisWeights.arena_deltas): the sums on delta arenas, no baseline
    _, _, rnd_p = make_round(None, deltas=True)
    wall, km = measure(lambda: rnd_p.np_sumsq(slots), rnd_p, ["np_sumsq"])
    out["polaris_sumsq"] = dict(entry(km["np_sumsq"], k * n_f * 4), path_ms=round(wall, 3),
                                kernel="plato_agg_np_sumsq, delta arenas",
                                staging_delta_ms_per_client=round(rnd_p.delta_ms_per_client, 4),
                                reference="examples/client_selection/polaris/polaris_server.py:78-81")
    out["polaris_sumsq_weight_arenas"] = dict(entry(km_w["np_sumsq"], (k + 1) * n_f * 4), path_ms=round(wall_w, 3),
                                              kernel="plato_agg_np_sumsq, weight arenas")
    del rnd_p
    torch.cuda.empty_cache()

    # QSGD-coded FedAvg: one code byte per element through HBM, decoded in the kernel
    qslab = ClientSlab(lay, k, dev, codec="qsgd")
    g = torch.Generator(device=dev).manual_seed(1)
    for r in range(k):  # what the client quantizer makes of normal deltas at level 64
        shape = qslab.f32[r].shape
        mag = torch.floor(torch.randn(shape, device=dev, generator=g).abs() * (63 / 5)
                          + torch.rand(shape, device=dev, generator=g)).clamp_(0, 127)
        sign = (torch.rand(shape, device=dev, generator=g) < 0.5).to(torch.float32) * 128
        qslab.f32[r].copy_((mag + sign).to(torch.uint8))
    qslab.i64.fill_(3)
    qpf, qpi = qslab.row_pointers(range(k))
    qtf, qti = torch.from_numpy(qpf).to(dev), torch.from_numpy(qpi).to(dev)
    n_e = len(lay.entries)
    max_v = torch.rand((n_e, k), device=dev, generator=g) * 0.1 + 0.01
    w = torch.full((k,), 1.0 / k, device=dev)
    cf, ci = rnd.engine._chunks(lay, rnd.engine.QSGD_CHUNK)
    out_f = torch.empty(lay.row_f32, device=dev)
    out_i = torch.empty(lay.row_i64, device=dev)
    stream = torch.cuda.current_stream(dev)

    def qsgd():
        _lib.call("plato_agg_fedavg_qsgd", _ptr(qtf), _ptr(qti), k, _ptr(max_v), n_e, 63.0, _ptr(w), None,
                  _ptr(cf), cf.shape[0], _ptr(ci), ci.shape[0], _ptr(base.f32), _ptr(base.i64), _ptr(out_f),
                  _ptr(out_i), lay.n_f32, n_i, stream.cuda_stream)

    qsgd()
    torch.cuda.synchronize(dev)
    ts = []
    for _ in range(max(reps, 10)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        qsgd()
        e1.record(stream)
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    out["qsgd_fedavg"] = dict(entry(statistics.median(ts), k * n_flat + 2 * model_bytes),
                              kernel="plato_agg_fedavg_qsgd",
                              reference="plato/processors/model_dequantize_qsgd.py:34-60 + servers/fedavg.py:137-159")
    del qslab, rnd
    torch.cuda.empty_cache()
    return out


# Strong scaling, N > 1: pieces per rank, chosen from the one-GPU anchor (``--anchor``).
# More pieces overlap more of the all-gather with the kernels but make each piece kernel smaller.
# From the one-GPU anchor with the one-wave kernel (profiles/r05d_anchor.log): a rank's
# kernels lose little to more pieces (C2 at N = 8: 0.116 ms in 1 piece, 0.123 in 4, 0.151 in 8), while
# each piece lets the all-gather of the one before it run under the kernels; with RCCL's all-gather
# modelled at one ~64 GB/s xGMI link for N = 2 and ~192 / ~330 GB/s of bus bandwidth for N = 4 / 8, plus
# ~15 us per collective, 4 pieces give the shortest step at every N for C2 and C3.
PIECES_BY_WORLD = {"C2": {2: 4, 4: 4, 8: 4}, "C3": {2: 4, 4: 4, 8: 4}}


def pieces_for(config: str, world: int) -> int:
    table = PIECES_BY_WORLD.get(config, PIECES_BY_WORLD["C2"])
    return table.get(world, table[max(table)])


def anchor_bench(args):
    """One rank's share of the strong-scaling job, timed on ONE GPU with no collective.

    For C2 and C3 and N = 1, 2, 4, 8 with 1, 2, 4, 8 pieces per rank: rank 0's pieces (the largest
    rank: it also carries the int64 entries) are launched back to back on one stream, exactly as
    ``main`` launches them at N > 1, over a slab laid out as the rank's (rows of pieces x piece
    length); HIP events around each piece and around the rank's whole step.  Also the headline
    kernel on C2-like arenas whose grids are 2 to 12 resident rounds (the grid-tail study of
    DESIGN.md §4).  Kernel variants from libplato_agg_tune.so (``--variant`` picks one), median of
    ``--steps`` interleaved repetitions.  Prints JSON lines; the all-gather a rank would add is
    reported as bytes (RCCL needs N distinct GPUs).
    """
    from plato_amd import _lib
    from plato_amd.arena import ArenaLayout
    from plato_amd.distributed import PiecePlan

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    nv = _lib.tune().plato_agg_tune_num_variants()
    variants = [args.variant] if args.variant is not None else [v for v in (0, 5, 11, 12, 13) if v < nv]
    reps = max(3, args.steps)

    def describe(v):
        import ctypes

        bs, a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _lib.tune().plato_agg_tune_describe(v, ctypes.byref(bs), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
        return {"B": bs.value, "V": a.value, "U": b.value, "persist": (c.value >> 4) & 255,
                "balanced": bool(c.value >> 13 & 1)}

    def run_shapes(label, k, shapes, row):
        """shapes: [(name, [(piece offset in the row, fp32 elements, int64 entries)], extra)] over one slab."""
        slab = torch.empty((k, row), dtype=torch.float32, device=dev)
        slab.uniform_(-1.0, 1.0)
        slab_i = torch.zeros((k, 64), dtype=torch.int64, device=dev)
        base = torch.empty(row, dtype=torch.float32, device=dev).uniform_(-1.0, 1.0)
        base_i = torch.zeros(64, dtype=torch.int64, device=dev)
        out = torch.empty(row, dtype=torch.float32, device=dev)
        out_i = torch.empty(64, dtype=torch.float32, device=dev)
        w = torch.full((k,), 1.0 / k, dtype=torch.float32, device=dev)
        ti = torch.from_numpy(slab_i.data_ptr() + np.arange(k, dtype=np.int64) * 64 * 8).to(dev)
        tables = {}

        def launch(v, pieces, stride=row):
            """``stride``: the client rows' pitch in floats (<= row: the slab's own, or a denser view of it)."""
            for off, n, ni in pieces:
                tf = tables.get((off, stride))
                if tf is None:
                    tf = tables[(off, stride)] = torch.from_numpy(
                        slab.data_ptr() + np.arange(k, dtype=np.int64) * stride * 4 + off * 4).to(dev)
                _lib.tune_call("plato_agg_tune_fedavg", v, 1, tf.data_ptr(), ti.data_ptr() if ni else None,
                               w.data_ptr(), None, k, base.data_ptr() + off * 4, base_i.data_ptr() if ni else None,
                               out.data_ptr() + off * 4, out_i.data_ptr() if ni else None, n, ni, stream.cuda_stream)

        if label == "grid_tail":  # what the timed loop's per-step HIP events cost (C2-sized launches)
            c2_pieces = next(p for name, p, _ in shapes if name.startswith("rounds_5.3"))
            gaps = {}
            for mode in ("none", "one", "three", "none"):
                marks = []
                launch(0, c2_pieces)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(reps * 5):
                    for _ in range({"none": 0, "one": 1, "three": 2}[mode]):
                        ev = torch.cuda.Event(enable_timing=True)
                        ev.record(stream)
                        marks.append(ev)
                    launch(0, c2_pieces)
                    if mode == "three":
                        ev = torch.cuda.Event(enable_timing=True)
                        ev.record(stream)
                        marks.append(ev)
                torch.cuda.synchronize(dev)
                gaps[mode] = min(gaps.get(mode, 1e9), (time.perf_counter() - t0) * 1e3 / (reps * 5))
            print(json.dumps({"anchor": "launch_gaps", "shape": "rounds_5.333", "clients": k,
                              "ms_per_launch_by_events_per_step": {m: round(v, 4) for m, v in gaps.items()},
                              "note": "wall clock over back-to-back launches; 'three' = bench.py's timed loop"}),
                  flush=True)
        for name, pieces, extra in shapes:
            nbytes = sum((k + 2) * (n * 4 + ni * 8) for _, n, ni in pieces)
            times = {v: [] for v in variants}
            stride = extra.get("row_stride", row)
            for v in variants:
                launch(v, pieces, stride)
            torch.cuda.synchronize(dev)
            for _ in range(reps):
                for v in variants:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    launch(v, pieces, stride)
                    e1.record(stream)
                    e1.synchronize()
                    times[v].append(e0.elapsed_time(e1))
            for v in variants:
                med = statistics.median(times[v])
                print(json.dumps({"anchor": label, "shape": name, "clients": k, "variant": v, **describe(v),
                                  "piece_elements": [n for _, n, _ in pieces], "algorithmic_bytes": nbytes,
                                  "kernel_ms": round(med, 4), "kernel_ms_min": round(min(times[v]), 4),
                                  "GBps": round(nbytes / (med * 1e-3) / 1e9, 1),
                                  "frac": round(nbytes / (med * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), **extra}),
                      flush=True)
        del slab, slab_i, base, out
        torch.cuda.empty_cache()

    # grid-tail study: C2's K on arenas of r resident rounds (256 CUs x 8 workgroups of 1,024 elements)
    per_round = 2048 * 1024
    c2 = ArenaLayout.from_shapes(model_spec("resnet18"))
    rounds = [2, 4, 5, c2.n_f32 / per_round, 5.5, 6, 8, 12]
    shapes = [(f"rounds_{r:.3f}", [(0, int(r * per_round) // 64 * 64, 0)], {"rounds": round(r, 3)}) for r in rounds]
    row = max(n for _, ((_, n, _),), _ in shapes)
    # C2 itself (with and without its int64 entries) at several client-row pitches: the bench's slab pitch
    # (the arena rounded to 64 floats), padded pitches and the power-of-two-multiple pitches above
    pitch = -(-c2.n_f32 // 64) * 64
    for stride in (pitch, pitch + 64, pitch + 1024, pitch + 4096, pitch + 32768, 12 * 2**20, 16 * 2**20, row):
        for ni in (c2.n_i64, 0):
            shapes.append((f"c2_pitch_{stride}_i64_{ni}", [(0, c2.n_f32, ni)],
                           {"row_stride": stride, "pitch_bytes": stride * 4, "int64_entries": ni}))
    run_shapes("grid_tail", 128, shapes, row)

    # one rank's pieces at N GPUs (rank 0: the largest bucket, with the int64 entries)
    for config in ("C2", "C3"):
        model, k = CONFIGS[config]
        full = ArenaLayout.from_shapes(model_spec(model))
        shapes, row = [], 0
        for world in (1, 2, 4, 8):
            for pieces in ((1,) if world == 1 else (1, 2, 4, 8)):
                plan = PiecePlan.for_layout(full, world, pieces)
                L = plan.length
                ps = [(p * L, plan.piece_elements(0, p), full.n_i64 if p == 0 else 0) for p in range(pieces)]
                ps = [x for x in ps if x[1] or x[2]]
                row = max(row, pieces * L)
                gather = world * (pieces * L + 64) * 4
                shapes.append((f"N{world}_p{pieces}", ps, {
                    "world": world, "pieces": pieces, "config": config,
                    "job_bytes": full.algorithmic_bytes(k),
                    "allgather_bytes_received_per_rank": (world - 1) * gather // world if world > 1 else 0}))
        progress(f"anchor {config}: {len(shapes)} layouts, slab {k} x {row} fp32 ({k * row * 4 / 1e9:.1f} GB)")
        run_shapes(config, k, shapes, row)


def engine_devices_bench(args):
    """The server's own multi-GPU path in one process (plato_amd.multi.MultiDeviceEngine).

    Host-inclusive: K CPU state_dicts -> native pack into pinned slots -> bucket g
    H2D to GPU g -> per-GPU kernel -> per-bucket D2H into one pinned result.
    Device-resident: the same rounds re-launched on staged inputs (kernels + D2H
    assembly), and with ``gather`` (RCCL all-gather; device copies when the box
    has fewer GPUs than buckets).  Prints one JSON line; not the driver's metric.
    """
    from plato_amd import synthetic
    from plato_amd import weights as W
    from plato_amd.arena import ArenaLayout
    from plato_amd.engine import ClientSlab, DeviceArena
    from plato_amd.multi import MultiDeviceEngine

    n = args.engine_devices
    count = torch.cuda.device_count()
    devices = [f"cuda:{g % count}" for g in range(n)]
    model, k_default = CONFIGS[args.config]
    k = args.clients or k_default
    layout = ArenaLayout.from_shapes(model_spec(model))
    dev0 = torch.device("cuda:0")
    base = DeviceArena(layout, dev0)
    slab = ClientSlab(layout, k, dev0)
    from plato_amd.synthetic import fill_baseline, fill_clients

    fill_baseline(base, args.seed)
    fill_clients(slab, base, args.seed, k)
    baseline, payloads = _host_state_dicts(layout, base, slab, k)
    del slab
    torch.cuda.empty_cache()
    weights = W.fedavg(synthetic.num_samples(k, args.seed))
    eng = MultiDeviceEngine(devices)
    bytes_ = layout.algorithmic_bytes(k)
    host, dev_only, gath = [], [], []
    for r in range(args.warmup + args.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rnd = eng.begin(baseline, k)
        rnd.put_baseline(baseline)
        for slot, p in enumerate(payloads):
            rnd.put_client(slot, p)
        rnd.launch(weights)
        rnd.result()
        t1 = time.perf_counter()
        if r >= args.warmup:
            host.append((t1 - t0, dict(rnd.timings)))
        # device-resident re-launch on the staged rows (kernels + assembly only)
        for gather, acc in ((False, dev_only), (True, gath)):
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            rnd.launch(weights, gather=gather)
            rnd.result()
            if r >= args.warmup:
                acc.append((time.perf_counter() - t2, dict(rnd.timings)))
    med = lambda xs: statistics.median(x[0] for x in xs)  # noqa: E731
    kern = lambda xs: statistics.median(x[1]["kernel_ms"] for x in xs)  # noqa: E731
    out = {
        "engine_devices": n, "devices": devices, "config": args.config, "clients": k,
        "algorithmic_bytes": bytes_,
        "host_inclusive": {"GBps": round(bytes_ / med(host) / 1e9, 2), "ms": round(med(host) * 1e3, 2),
                           "stage_ms": round(statistics.median(x[1]["stage_ms"] for x in host), 2),
                           "kernel_ms_max": round(kern(host), 4)},
        "device_resident_host_result": {"GBps": round(bytes_ / med(dev_only) / 1e9, 1),
                                        "ms": round(med(dev_only) * 1e3, 3), "kernel_ms_max": round(kern(dev_only), 4)},
        "device_resident_gathered": {"GBps": round(bytes_ / med(gath) / 1e9, 1), "ms": round(med(gath) * 1e3, 3)},
        "note": "median over --steps rounds after --warmup; repeated devices share one GPU",
    }
    if args.client_split:
        out["client_split"] = client_split_leg(eng, baseline, payloads, k, args.steps)
    if args.parity:
        out.update(engine_devices_parity(eng, layout, baseline, payloads, weights))
    out["rccl_communicator"] = eng._comm is not None  # ncclCommInitAll over distinct GPUs
    print(json.dumps(out), flush=True)
    eng.close()
    if str(out.get("parity", "")).startswith("MISMATCH"):
        sys.exit(3)


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    a, b = a.reshape(-1), b.reshape(-1)
    if a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    return torch.equal(a, b)


def engine_devices_parity(eng, layout, baseline, payloads, weights) -> dict:
    """MultiDeviceEngine's host result and every GPU's gathered copy against the one-GPU engine, bit for bit.

    One more round of the multi-device engine with ``gather=True`` (RCCL all-gather over distinct GPUs,
    device copies where devices repeat); the reference is ``FedAvgEngine`` on the first device with the
    same baseline, payloads and weights — the product path at N = 1, which the golden fixtures pin.
    """
    from plato_amd.arena import F32
    from plato_amd.engine import FedAvgEngine

    one = FedAvgEngine(eng.devices[0]).aggregate_weights(baseline, payloads, weights)
    rnd = eng.begin(baseline, len(payloads))
    rnd.put_baseline(baseline)
    for slot, p in enumerate(payloads):
        rnd.put_client(slot, p)
    rnd.launch(weights, gather=True)
    host = rnd.result()
    bad_host = [n for n in one if not _same_bits(one[n], host[n])]
    bad_dev = []
    for g in range(eng.world):
        f, i = rnd.device_result(g)
        f, i = f.cpu(), i.cpu()
        for e in layout.entries:
            # fp32 entries, and the int64 entries' fp32 results (update_weights' values, before load_weights)
            got = (f if e.region == F32 else i)[e.offset:e.offset + e.numel]
            if not _same_bits(got, one[e.name]):
                bad_dev.append((g, e.name))
    exact = not bad_host and not bad_dev
    return {"parity": "bit-exact vs 1-GPU engine (host result and every GPU's gathered copy)" if exact
            else "MISMATCH vs 1-GPU engine",
            "parity_detail": {"entries": len(layout.entries), "gathered_copies_checked": eng.world,
                              "host_mismatched_entries": bad_host[:8],
                              "device_mismatched": [f"gpu{g}:{n}" for g, n in bad_dev[:8]]}}


def client_split_leg(eng, baseline, payloads, k: int, reps: int) -> dict:
    """FedAdp over the multi engine's devices split by client (``ClientRound``): the asynchronous assembly of
    each device's client arenas from the bucket shards, then the global gradient and the dots."""
    asm_wall, asm_dev, dots = [], [], []
    w1 = None
    for r in range(reps + 1):
        rnd = eng.clients.begin(baseline, k)
        rnd.put_baseline(baseline)
        for slot, p in enumerate(payloads):
            rnd.put_client(slot, p)
        for d in dict.fromkeys(eng.devices):
            torch.cuda.synchronize(d)
        t0 = time.perf_counter()
        rnd._client_rounds()
        for d in dict.fromkeys(eng.devices):
            torch.cuda.synchronize(d)
        t1 = time.perf_counter()
        rnd._resolve_assembly()
        if w1 is None:
            w1 = np.full((len(rnd.layout.entries), k), 1.0 / k)
        t2 = time.perf_counter()
        grads = rnd.launch_entrywise(w1, add_base=False, device=True)
        rnd.fedadp_dots(grads, list(range(k)), 0.01)
        t3 = time.perf_counter()
        if r:
            asm_wall.append((t1 - t0) * 1e3)
            asm_dev.append(rnd.timings["client_assembly_ms"])
            dots.append((t3 - t2) * 1e3)
        del rnd
    per_dev = eng.world
    moved = sum(p_.numel() * p_.element_size() for p_ in payloads[0].values()) * k
    med = statistics.median
    return {"clients": k, "devices": per_dev, "client_bytes_moved": moved,
            "client_assembly_ms": round(med(asm_dev), 3), "client_assembly_wall_ms": round(med(asm_wall), 3),
            "client_assembly_GBps": round(moved / (med(asm_dev) * 1e-3) / 1e9, 1),
            "fedadp_entrywise_and_dots_wall_ms": round(med(dots), 3),
            "note": "one strided device-to-device copy per (device, bucket); repeated devices share one GPU, so the "
                    "copies are HBM-to-HBM on it (xGMI on a real node); median of --steps after one warm-up"}


def _host_state_dicts(layout, base, slab, k):
    bf = base.f32[: layout.n_f32].cpu()
    bi = base.i64[: layout.n_i64].cpu()
    baseline = layout.unpack(bf, bi)
    payloads = []
    for c in range(k):
        payloads.append(layout.unpack(slab.f32[c, : layout.n_f32].cpu(), slab.i64[c, : layout.n_i64].cpu()))
    return baseline, payloads


def host_inclusive(engine, layout, base, slab, k, weights, dev):
    """CPU state_dicts in -> CPU state_dict out through the engine (pack, H2D, kernel, D2H)."""
    if k * (layout.n_f32 * 4 + layout.n_i64 * 8) > 16e9:
        return None  # would need the whole job's payloads in host memory
    baseline, payloads = _host_state_dicts(layout, base, slab, k)
    times = []
    for _ in range(3):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        engine.aggregate_weights(baseline, payloads, weights)
        torch.cuda.synchronize(dev)
        times.append(time.perf_counter() - t0)
    med = statistics.median(times[1:])
    out = {"value": round(layout.algorithmic_bytes(k) / med / 1e9, 2), "unit": "GB/s",
           "ms": round(med * 1e3, 2),
           "note": "pack CPU state_dicts -> pinned -> H2D -> kernel -> D2H; median of 2 after 1 warm-up"}
    # from the wire: pickled payload bytes (what the server receives, servers/base.py:821)
    import pickle

    from plato_amd import ingest

    # clients pickle model.state_dict(): one storage per tensor (views of one
    # arena would each serialise the whole arena)
    wire = [pickle.dumps(type(p)((n, t.clone()) for n, t in p.items())) for p in payloads]
    del payloads
    t_wire = []
    t_pickle = None
    for r in range(3):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        rnd = engine.begin(baseline, k)
        rnd.put_baseline(baseline)
        for slot, data in enumerate(wire):
            rnd.put_client(slot, ingest.loads(data, layout=layout, pin=True))
        rnd.launch(weights)
        rnd.result()
        t_wire.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    for data in wire[:8]:
        pickle.loads(data)
    t_pickle = (time.perf_counter() - t0) / 8
    # as the socket delivers it: 1 MiB chunks (servers/base.py:728-736, joined at :821)
    chunked = [[d[i:i + 2**20] for i in range(0, len(d), 2**20)] for d in wire[:8]]
    t0 = time.perf_counter()
    for ch in chunked:
        pickle.loads(b"".join(ch))
    t_ref_chunks = (time.perf_counter() - t0) / 8
    ingest.loads_chunks(chunked[0], layout=layout, pin=True)
    t0 = time.perf_counter()
    for ch in chunked:
        ingest.loads_chunks(ch, layout=layout, pin=True)
    t_chunks = (time.perf_counter() - t0) / 8
    # comm_simulation (Plato's default): the payload arrives as a file the client
    # pickle.dump'ed (clients/base.py:372-386), pickle.load'ed at servers/base.py:791-792
    import tempfile

    with tempfile.NamedTemporaryFile(suffix=".pth") as f:
        f.write(wire[0])
        f.flush()
        t_file_ref, t_file = [], []
        for _ in range(4):
            t0 = time.perf_counter()
            with open(f.name, "rb") as fh:
                pickle.load(fh)
            t_file_ref.append(time.perf_counter() - t0)
        ingest.load_file(f.name, layout=layout, pin=True)
        for _ in range(4):
            t0 = time.perf_counter()
            ingest.load_file(f.name, layout=layout, pin=True)
            t_file.append(time.perf_counter() - t0)
    # size accounting: the reference re-pickles each payload to log its size
    # (servers/base.py:839-846); WireIngestMixin takes the wire length instead
    loaded = [pickle.loads(d) for d in wire[:4]]
    t0 = time.perf_counter()
    for p in loaded:
        sys.getsizeof(pickle.dumps(p))
    t_resize = (time.perf_counter() - t0) / len(loaded)
    del loaded
    med_w = statistics.median(t_wire[1:])
    out["from_wire"] = {
        "value": round(layout.algorithmic_bytes(k) / med_w / 1e9, 2), "unit": "GB/s",
        "ms": round(med_w * 1e3, 2),
        "native_parse_ms_per_payload": round(med_w * 1e3 / k, 3),
        "pickle_loads_ms_per_payload": round(t_pickle * 1e3, 3),
        "socket_chunks": {"reference_join_pickle_loads_ms": round(t_ref_chunks * 1e3, 3),
                          "native_join_parse_gather_ms": round(t_chunks * 1e3, 3)},
        "comm_simulation_file": {"reference_pickle_load_ms": round(statistics.median(t_file_ref) * 1e3, 3),
                                 "native_read_parse_gather_ms": round(statistics.median(t_file) * 1e3, 3)},
        "size_accounting": {"reference_repickle_ms": round(t_resize * 1e3, 3), "native": "wire length, no copy"},
        "note": "pickled payload bytes -> libplato_ingest parse + gather into pinned arenas -> H2D -> "
                "kernel -> D2H (replaces pickle.loads at servers/base.py:822)"}
    return out


def streaming(engine, layout, base, slab, k, weights, dev, reps=3):
    """Async servers: stage each payload to HBM as it arrives, reduce at the trigger.

    * arrival staging: K CPU state_dicts staged back to back (FedAvgEngine.prestage:
      pack into the pinned ring, H2D on the copy stream), GB/s of payload bytes;
    * trigger-to-result: the first K-1 payloads arrived (and were staged) earlier;
      the last one arrives, then the round adopts every staged slot in
      ``self.updates`` order, launches and returns the CPU state_dict — the
      latency the server sees after the last report.
    """
    from plato_amd.arena import ArenaLayout

    baseline, payloads = _host_state_dicts(layout, base, slab, k)
    blay = ArenaLayout.from_state_dict(baseline)
    per_client = layout.n_f32 * 4 + layout.n_i64 * 8
    stage_s, trig_s = [], []
    for r in range(reps + 1):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for p in payloads[:-1]:
            engine.prestage(p, blay)
        engine._copy_stream.synchronize()
        t1 = time.perf_counter()
        engine.prestage(payloads[-1], blay)  # the last report: trigger
        rnd = engine.begin(baseline, k)
        rnd.put_baseline(baseline)
        for slot, p in enumerate(payloads):
            if not rnd.adopt(slot, p):
                raise RuntimeError("payload was not staged on arrival")
        rnd.launch(weights)
        rnd.result()
        t2 = time.perf_counter()
        engine.release_arrivals()
        if r:
            stage_s.append(t1 - t0)
            trig_s.append(t2 - t1)
    st = statistics.median(stage_s)
    return {
        "clients": k,
        "arrival_staging_GBps": round((k - 1) * per_client / st / 1e9, 2),
        "arrival_staging_ms_per_payload": round(st / (k - 1) * 1e3, 3),
        "trigger_to_result_ms": round(statistics.median(trig_s) * 1e3, 2),
        "note": "CPU state_dicts staged to HBM on arrival (pack -> pinned -> H2D); trigger-to-result = last "
                "payload's staging + baseline H2D + kernel + D2H of the new state_dict; median of "
                f"{reps} after 1 warm-up",
    }


def cpu_baseline(layout, base, slab, k, weights, out_f, out_i, reps, config):
    """Reference op sequence (oracle port) on the host on a bounded sample of the job.

    The sample is the first k_s clients of the same device inputs (all K for
    C2), sized to ~6 GB of client payload so the leg stays within tens of
    seconds; the GPU result is checked bit for bit when k_s == K.
    """
    from oracle import fedavg_oracle as ref

    per_client = layout.n_f32 * 4 + layout.n_i64 * 8
    k_s = max(1, min(k, int(6e9 // max(per_client, 1))))
    baseline, payloads = _host_state_dicts(layout, base, slab, k_s)
    w_s = weights[:k_s]
    default_threads = torch.get_num_threads()
    # time the reference sequence with the host's CPUs as well as torch's
    # default pool; the CPUs this process may use (nproc counts the whole machine)
    avail = cpus_available() or default_threads
    # nproc counts the whole machine; a pool that size under the job's CPU quota oversubscribes it
    # (a 256-thread pass on a 16-CPU quota ran for minutes), so it is reported, not timed
    nproc = os.cpu_count() or avail
    by_threads = {}
    upd = None
    for threads in sorted({default_threads, avail}):
        progress(f"cpu baseline: {k_s} clients on {threads} threads")
        torch.set_num_threads(threads)
        times = []
        for r in range(reps + 1):
            t0 = time.perf_counter()
            upd = ref.fedavg_torch_ops(baseline, payloads, weights=w_s)
            dt = time.perf_counter() - t0
            if r or dt > 20:  # a slow pool: its first pass is the measurement (bounded leg)
                times.append(dt)
            if dt > 20:
                break
        by_threads[threads] = statistics.median(times)
    torch.set_num_threads(default_threads)
    threads = min(by_threads, key=by_threads.get)  # the faster pool is the baseline
    med = by_threads[threads]
    parity = "not checked (sampled subset of clients)"
    if k_s == k:
        gpu_f = out_f[: layout.n_f32].cpu()
        gpu_i = out_i[: layout.n_i64].cpu()
        exp_f = torch.cat([upd[e.name].reshape(-1) for e in layout.entries if e.region == "f32"])
        exp_i = torch.cat([upd[e.name].reshape(-1) for e in layout.entries if e.region == "i64"]) \
            if layout.n_i64 else torch.empty(0)
        exact = bool(torch.equal(gpu_f.view(torch.int32), exp_f.view(torch.int32))
                     and torch.equal(gpu_i.view(torch.int32), exp_i.view(torch.int32)))
        parity = "bit-exact vs CPU reference op sequence" if exact else "MISMATCH vs CPU reference"
    # the same sequence on 1 thread (first 8 clients), and the
    # host's STREAM-style copy rate (1 GiB fp32, read + write bytes) at `threads`
    k1 = min(k_s, 8)
    t1 = []
    torch.set_num_threads(1)
    try:
        for r in range(3):
            t0 = time.perf_counter()
            ref.fedavg_torch_ops(baseline, payloads[:k1], weights=w_s[:k1])
            if r:
                t1.append(time.perf_counter() - t0)
    finally:
        torch.set_num_threads(default_threads)
    src = torch.ones(1 << 28, dtype=torch.float32)
    dst = torch.empty_like(src)
    tc = []
    for r in range(4):
        t0 = time.perf_counter()
        dst.copy_(src)
        if r:
            tc.append(time.perf_counter() - t0)
    stream_gbps = 2 * src.numel() * 4 / statistics.median(tc) / 1e9
    del src, dst
    return {
        "value": round(layout.algorithmic_bytes(k_s) / med / 1e9, 3),
        "unit": "GB/s",
        "cores": threads,
        "by_threads": {str(t): round(layout.algorithmic_bytes(k_s) / v / 1e9, 3) for t, v in by_threads.items()},
        "cpus_available": avail,
        "nproc": nproc,
        "kind": "port",
        "one_thread": {"value": round(layout.algorithmic_bytes(k1) / statistics.median(t1) / 1e9, 3),
                       "unit": "GB/s", "sample": f"first {k1} clients, median of 2 after 1 warm-up"},
        "host_copy_GBps": round(stream_gbps, 1),
        "sample": f"{config}: {k_s} of {k} clients x {layout.n_f32 + layout.n_i64} params; the "
                  f"reference's torch CPU op sequence sub->mul->add_->add per tensor, median of {reps} "
                  f"after 1 warm-up, {threads} threads on {cpu_model()} (nproc {os.cpu_count()})",
        "ms": round(med * 1e3, 1),
        "parity": parity,
    }


if __name__ == "__main__":
    main()
