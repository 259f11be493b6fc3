"""Device engine: HBM arenas, host staging and launches of the HIP kernels.

This is the host half of the drop-in boundary.  It takes what Plato's server
hands to its aggregation hooks (CPU ``state_dict`` payloads in
``self.updates`` order, the baseline from ``algorithm.extract_weights()``,
per-client weights) and returns what the reference would return, computed by
``libplato_agg.so`` on the GPU:

* :meth:`FedAvgEngine.aggregate_weights` — the fused deltas -> weighted sum ->
  update chain (``plato/servers/fedavg.py:184-194``), i.e. the value an
  ``aggregate_weights`` hook must produce (``servers/fedavg.py:171-182``).
* :meth:`FedAvgEngine.aggregate_deltas` — ``Server.aggregate_deltas``
  (``servers/fedavg.py:137-159``) for variants that compute their own deltas.
* :meth:`FedAvgEngine.compute_weight_deltas` / :meth:`update_weights` /
  :meth:`mix_weights` — ``algorithms/fedavg.py:13-37`` and FedAsync's
  ``fedasync_algorithm.py:9-20``.

Everything device-side goes through the C ABI; nothing here computes model
arithmetic on the CPU.
"""

from __future__ import annotations

import time
from collections import OrderedDict
from typing import Mapping, Sequence

import numpy as np
import torch

from . import _lib
from .arena import CODECS, F32, I64, ArenaLayout, DeviceArena, payload_codec, same_f32_bits
from .arrivals import Adopt, ArrivalTable, adopt_rule
from .elastic import ElasticAggregates
from .reductions import VariantLaunches
from .robust import RobustAggregates, RobustLaunches
from .staging import HostPacker, PinnedRing, ResultPool, arena_source, baseline_key, payload_fingerprint
from .submodel import SubmodelAggregates


def fp32_weights(values: Sequence[float]) -> np.ndarray:
    """Round Python (double) weights to fp32 the way torch's scalar path does.

    ``delta * (n_i / N)`` multiplies an fp32 tensor by a Python float; torch
    converts the double scalar to the fp32 compute type (round to nearest even)
    before the multiply (measured).
    """
    out = np.empty(len(values), dtype=np.float32)
    for i, v in enumerate(values):
        if isinstance(v, torch.Tensor):
            raise TypeError("aggregation weights must be Python numbers, not tensors")
        out[i] = np.float32(float(v))
    return out


def fedavg_weights(num_samples: Sequence[int]) -> list[float]:
    """``n_i / N`` as the reference computes it (``servers/fedavg.py:140,154``)."""
    total = sum(num_samples)
    return [n / total for n in num_samples]


def require_device(device=None) -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError(
            "plato_amd: no ROCm GPU visible; the aggregation engine runs only on the "
            "HIP path (there is no CPU fallback)"
        )
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"plato_amd: device must be a GPU, got {dev}")
    return dev


def staged_slots(capacity: int, staged: Sequence[bool], slots: Sequence[int]) -> list[int]:
    """``slots`` as a list, every one of them in range and staged (single- and multi-GPU rounds)."""
    slots = list(slots)
    for slot in slots:
        if not (0 <= slot < capacity and staged[slot]):
            raise ValueError(f"client slot {slot} was not staged")
    return slots


def _ptr(t: torch.Tensor | None) -> int | None:
    return None if t is None else t.data_ptr()


def _stream_handle(stream: torch.cuda.Stream) -> int:
    return stream.cuda_stream


class ClientSlab:
    """K client arenas in HBM as two row-major slabs ``[cap, row]``.

    ``codec`` selects the element types the payloads arrive in (arena.CODECS):
    bf16 payloads stay bf16 in HBM (half the bytes) and are widened by the kernel.
    """

    def __init__(self, layout: ArenaLayout, capacity: int, device: torch.device, codec: str = "native"):
        self.layout = layout
        self.capacity = capacity
        self.codec = codec
        dt_f, dt_i = CODECS[codec]
        self.f32 = torch.empty((capacity, layout.row_f32), dtype=dt_f, device=device)
        self.i64 = torch.empty((capacity, layout.row_i64), dtype=dt_i, device=device)

    def row_pointers(self, rows: Sequence[int]) -> tuple[np.ndarray, np.ndarray]:
        base_f = self.f32.data_ptr()
        base_i = self.i64.data_ptr()
        sf = self.f32.stride(0) * self.f32.element_size()
        si = self.i64.stride(0) * self.i64.element_size()
        rows = np.asarray(rows, dtype=np.int64)
        return (base_f + rows * sf).astype(np.int64), (base_i + rows * si).astype(np.int64)


class _Stager:
    """Pinned host ring: packs CPU ``state_dict``s natively and copies them H2D.

    Packing client j+1 (``plato_ingest_pack`` on the native copy pool) overlaps
    the H2D copy of client j on a dedicated copy stream; arena-backed payloads
    (native ingestion) are copied from their pinned arena without a pack.
    """

    def __init__(self, layout: ArenaLayout, device: torch.device, depth: int = 4, codec: str = "native",
                 stream: torch.cuda.Stream | None = None):
        self.layout = layout
        self.codec = codec
        self.stream = stream or torch.cuda.Stream(device)
        self.ring = PinnedRing(layout, codec, depth)
        self.packer = HostPacker(layout, codec)

    def put(self, state_dict: Mapping[str, torch.Tensor], dst_f32: torch.Tensor,
            dst_i64: torch.Tensor) -> None:
        n_f, n_i = self.layout.n_f32, self.layout.n_i64
        src = arena_source(state_dict, self.layout, self.codec)
        if src is not None:
            # already laid out as the arena, in pinned memory (plato_amd.ingest.loads): DMA it as is
            arena_f, arena_i = src
            with torch.cuda.stream(self.stream):
                if n_f:
                    dst_f32[:n_f].copy_(arena_f[:n_f], non_blocking=True)
                if n_i:
                    dst_i64[:n_i].copy_(arena_i[:n_i], non_blocking=True)
            return
        with self.ring.lock:  # acquire -> pack -> copy -> fence as one step (executor vs event loop)
            j = self.ring.acquire()
            hf, hi = self.ring.slots[j]
            self.packer.pack(state_dict, hf, hi)
            with torch.cuda.stream(self.stream):
                if n_f:
                    dst_f32[:n_f].copy_(hf[:n_f], non_blocking=True)
                if n_i:
                    dst_i64[:n_i].copy_(hi[:n_i], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(self.stream)
            self.ring.fence(j, [ev])

    def fence(self, stream: torch.cuda.Stream) -> None:
        """Make ``stream`` wait for every copy issued so far."""
        stream.wait_stream(self.stream)


class FedAvgEngine(RobustAggregates, SubmodelAggregates, ElasticAggregates):
    """HIP FedAvg aggregation on one GPU (one process per GPU); the detector example's robust
    aggregators are ``plato_amd.robust``'s, the model-search examples' sub-model means ``plato_amd.submodel``'s and
    ``plato_amd.elastic``'s."""

    #: QSGD kernel variant (tuning / tests; None = the library default)
    qsgd_variant: int | None = None
    port_variant: int | None = None  # plato_agg_tune_port_norms shape (tests / tuning), None = the default
    #: arena alignment of the layouts this engine builds (arena.ALIGNMENTS; FedAdp servers: "fedadp")
    layout_align: str | None = None
    #: native rounds hold each client as its delta x - b (``AggregationRound.deltas``): FedAdp's servers,
    #: whose dot kernel then streams no baseline
    delta_arenas: bool = False

    def __init__(self, device=None, variant: int | None = None):
        self.device = require_device(device)
        self.lib = _lib.lib()
        self.variant = variant
        self._layout: ArenaLayout | None = None
        self._slabs: dict[str, ClientSlab] = {}
        self._stagers: dict[str, _Stager] = {}
        self._base: DeviceArena | None = None
        self._copy_stream: torch.cuda.Stream | None = None
        self._side: torch.cuda.Stream | None = None
        self._slab: ClientSlab | None = None      # slab of the current round's codec
        self._stager: _Stager | None = None       # native-dtype stager (baselines)
        self._arrivals = ArrivalTable()           # id(payload) -> Arrival; rows: its (fp32, int64) row pointers
        self._arrival_slabs: dict = {}
        self._arrival_base: DeviceArena | None = None  # the model arrivals are turned into deltas against
        self._submodel = None                     # plato_amd.submodel's layouts, stagers and slab
        self._elastic = None                      # plato_amd.elastic's
        self.fldetector = None                    # plato_amd.detectors.FLDetectorState, kept across rounds

    # ----------------------------------------------------------- allocation
    def _prepare(self, template: Mapping[str, torch.Tensor], k: int, codec: str = "native") -> ArenaLayout:
        if codec not in CODECS:
            raise ValueError(f"unknown payload codec {codec!r}")
        layout = self._use_layout(ArenaLayout.from_state_dict(template, align=self.layout_align), codec)
        slab = self._slabs.get(codec)
        if slab is None or slab.capacity < k:
            self._slabs.pop(codec, None)
            slab = ClientSlab(layout, k, self.device, codec)
            self._slabs[codec] = slab
        if self._base is None:
            self._base = DeviceArena(layout, self.device)
        self._slab = slab
        self._stager = self._stagers["native"]
        return layout

    def _use_layout(self, layout: ArenaLayout, codec: str) -> ArenaLayout:
        """The engine's layout: ``layout`` if its signature is new (arenas, stagers and arrivals of the old
        one are dropped), with the copy stream and the native and ``codec`` stagers in place."""
        if self._layout is None or self._layout.signature != layout.signature:
            self._layout = layout
            self._slabs, self._stagers, self._base = {}, {}, None
            self._arrivals.reset()
            self._arrival_slabs, self._arrival_base = {}, None
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(self.device)
        for c in {"native", codec}:
            if c not in self._stagers:
                self._stagers[c] = _Stager(self._layout, self.device, codec=c, stream=self._copy_stream)
        return self._layout

    def _upload_weights(self, weights: Sequence[float], scales: Sequence[float] | None):
        w = torch.from_numpy(fp32_weights(weights)).to(self.device, non_blocking=False)
        s = None
        if scales is not None:
            if len(scales) != len(weights):
                raise ValueError("scales must have one entry per client")
            s = torch.from_numpy(fp32_weights(scales)).to(self.device, non_blocking=False)
        return w, s

    def _pointer_tables(self, pf: np.ndarray, pi: np.ndarray):
        tf = torch.from_numpy(pf).to(self.device)
        ti = torch.from_numpy(pi).to(self.device)
        return tf, ti

    # per-entry kernels: chunk capacity (elements) per workgroup
    STATS_CHUNK = 4096      # entry_stats: 256 lanes x 4 float4 groups
    QSGD_CHUNK = 4096       # fedavg_qsgd: 256 lanes x 2 x 8 one-byte codes (plato_agg_tune_qsgd_chunk(29))
    ENTRYWISE_CHUNK = 256  # fedavg_entrywise: 64 lanes x 1 float4 group (round 5: 0.891 vs 0.917 ms for 256 x 2, r05i_entrywise.log)

    def _chunks(self, layout: ArenaLayout, cap: int):
        """Device copies of ``layout.chunk_tables(cap)`` (cached per layout)."""
        key = ("dev_chunks", cap, str(self.device))
        hit = layout._cache.get(key)
        if hit is None:
            cf, ci = layout.chunk_tables(cap)
            hit = (torch.from_numpy(cf.view(np.int32).copy()).to(self.device),
                   torch.from_numpy(ci.view(np.int32).copy()).to(self.device))
            layout._cache[key] = hit
        return hit

    def _norm_tables(self, layout: ArenaLayout):
        """One piece per entry, longest first (``plato_agg_entry_norms_f32``).

        Each (client, entry) norm is one serial fma chain (torch's CPU order),
        so the launch lasts at least as long as the longest chain; starting the
        longest entries first lets the short ones fill in behind them instead
        of delaying them (ResNet's largest convolutions come last in
        ``state_dict`` order).  The output is indexed by each piece's entry, so
        the table order changes only the schedule.
        """
        key = ("dev_norm_tables", str(self.device))
        hit = layout._cache.get(key)
        if hit is None:
            ef, ei = layout.chunk_tables(1 << 32)
            ef = ef[np.argsort(-(ef[:, 2].astype(np.int64) - ef[:, 1]), kind="stable")] if len(ef) else ef
            hit = (torch.from_numpy(np.ascontiguousarray(ef).view(np.int32).copy()).to(self.device),
                   torch.from_numpy(np.ascontiguousarray(ei).view(np.int32).copy()).to(self.device))
            layout._cache[key] = hit
        return hit

    #: fp32 entries at least this long get their per-(entry, client) norms from plato_agg_port_norms
    #: on a side stream (FedAtt); None (the default) = every entry through plato_agg_entry_norms_f32.
    #: Measured on 128 ResNet-18 clients: 1.45 ms with None, 1.71-2.15 ms with thresholds of 2^15-2^20
    #: (profiles/r03t_fedatt.log)
    norms_long_threshold: int | None = None

    def side_stream(self) -> torch.cuda.Stream:
        if self._side is None:
            self._side = torch.cuda.Stream(self.device)
        return self._side

    def _norm_tables_without(self, layout: ArenaLayout, drop: tuple) -> torch.Tensor:
        """The fp32 norm table (longest first) without the entries in ``drop``."""
        key = ("dev_norm_tables_without", drop, str(self.device))
        hit = layout._cache.get(key)
        if hit is None:
            ef, _ = layout.chunk_tables(1 << 32)
            ef = ef[np.argsort(-(ef[:, 2].astype(np.int64) - ef[:, 1]), kind="stable")] if len(ef) else ef
            ef = ef[~np.isin(ef[:, 0].astype(np.int64), np.asarray(drop, dtype=np.int64))] if len(ef) else ef
            hit = torch.from_numpy(np.ascontiguousarray(ef).view(np.int32).copy()).to(self.device)
            layout._cache[key] = hit
        return hit

    def _result_pool(self, layout: ArenaLayout) -> ResultPool:
        pool = layout._cache.get("result_pool")
        if pool is None:
            pool = layout._cache["result_pool"] = ResultPool(layout)
        return pool

    def _f32_stager(self, layout: ArenaLayout | None = None) -> "_Stager":
        """All-fp32 arrays over the model's keys (FedAtt's noise), packed in ``layout`` (default: the engine's)."""
        if layout is None or layout is self._layout:
            st = self._stagers.get("f32")
            if st is None:
                st = _Stager(self._layout, self.device, codec="f32", stream=self._copy_stream)
                self._stagers["f32"] = st
            return st
        st = layout._cache.get(("f32_stager", str(self.device)))
        if st is None:
            st = layout._cache[("f32_stager", str(self.device))] = _Stager(layout, self.device, codec="f32",
                                                                           stream=self._copy_stream)
        return st

    # ---------------------------------------------------- arrival staging
    ARRIVAL_CHUNK = 16  # rows per arrival slab; rows never move once staged

    def _grow_arrivals(self, codec: str) -> list:
        slab = ClientSlab(self._layout, self.ARRIVAL_CHUNK, self.device, codec)
        self._arrival_slabs.setdefault(codec, []).append(slab)
        return [(slab, r) for r in range(self.ARRIVAL_CHUNK)]

    def prestage(self, payload: Mapping[str, torch.Tensor], baseline_layout: ArenaLayout,
                 baseline: Mapping[str, torch.Tensor] | None = None) -> bool:
        """Copy one arriving payload to HBM now (H2D overlaps the other clients' arrival).

        The next aggregation round adopts it by identity (``AggregationRound.adopt``; the bookkeeping is
        ``plato_amd.arrivals``); the payload must not be modified after arrival.  Returns False if the
        payload does not fit the layout (it is then staged at aggregation time).  With :attr:`delta_arenas`
        and the server's current model as ``baseline`` (the baseline of the round this payload will join),
        the row is turned into its delta right behind its H2D; a round adopts it only if its own baseline
        is that model unchanged (``arrivals.adopt_rule``), else it stages the payload again.
        """
        codec = payload_codec(payload)
        try:
            baseline_layout.check_compatible(payload, "arriving payload", codec)
        except (KeyError, ValueError):
            return False
        self._use_layout(baseline_layout, codec)
        slab, row = self._arrivals.take(codec, lambda: self._grow_arrivals(codec))
        self._stagers[codec].put(payload, slab.f32[row], slab.i64[row])
        pf, pi = (int(p[0]) for p in slab.row_pointers([row]))
        delta_key = None
        if self.delta_arenas and codec == "native" and baseline is not None:
            delta_key = self._arrivals.baseline(baseline, self._layout, self._stage_arrival_base)
            if delta_key is not None:  # x - b in place, behind this payload's H2D on the copy stream
                self._to_delta(pf, pi, self._arrival_base, self._copy_stream)
        self._arrivals.file(payload, codec, self._layout.signature, (pf, pi), (slab, row), delta_key)
        return True

    def _to_delta(self, pf: int, pi: int, base: DeviceArena, stream: torch.cuda.Stream) -> None:
        """The row at (``pf``, ``pi``) becomes x - ``base``, in place, on ``stream`` (behind the row's H2D)."""
        lay = base.layout
        n_i = lay.n_i64
        _lib.call("plato_agg_compute_deltas", pf, pi if n_i else None, _ptr(base.f32), _ptr(base.i64) if n_i else None,
                  pf, pi if n_i else None, lay.n_f32, n_i, _stream_handle(stream))

    def _stage_arrival_base(self, model: Mapping[str, torch.Tensor]) -> None:
        """``model`` as the arrival baseline on the device (``ArrivalTable.baseline``: once per model version)."""
        if self._arrival_base is None:
            self._arrival_base = DeviceArena(self._layout, self.device)
        self._stagers["native"].put(model, self._arrival_base.f32, self._arrival_base.i64)

    def drop_arrival(self, payload) -> None:
        """Return one payload's arrival slot (a multi-GPU prestage that failed on another device).

        A copy still in flight into the row is ordered before any later copy into it (one copy stream)."""
        self._arrivals.drop(payload)

    def refresh_arrival(self, payload) -> None:
        """``payload``'s staged row was changed on the device and the payload written to match it (the
        attack simulation's write-back): its record follows the payload's new version counters, so the
        next round still adopts the row."""
        rec = self._arrivals.get(id(payload))
        if rec is not None and rec.payload is payload:
            rec.fingerprint = payload_fingerprint(payload)

    def release_arrivals(self) -> None:
        """Return every arrival slot (after the round that used them has completed, or failed)."""
        self._arrivals.release()

    # ------------------------------------------------------ raw device call
    def launch_fedavg(self, layout: ArenaLayout, ptr_f32: torch.Tensor, ptr_i64: torch.Tensor | None,
                      w: torch.Tensor, s: torch.Tensor | None, k: int,
                      base_f32: torch.Tensor | None, base_i64: torch.Tensor | None,
                      out_f32: torch.Tensor, out_i64f: torch.Tensor | None,
                      stream: torch.cuda.Stream | None = None) -> None:
        """Launch the fused kernel on device-resident arenas (no host traffic).

        ``base_f32 is None`` selects deltas mode (``aggregate_deltas``).
        """
        stream = stream or torch.cuda.current_stream(self.device)
        n_f, n_i = layout.n_f32, layout.n_i64
        if ptr_f32.numel() < k or w.numel() < k:
            raise ValueError("pointer table / weights shorter than K")
        args_tail = (n_f, n_i, _stream_handle(stream))
        ptr_i = _ptr(ptr_i64) if n_i else None
        if self.variant is None:
            if base_f32 is not None:
                _lib.call("plato_agg_fedavg_weights", _ptr(ptr_f32), ptr_i, _ptr(w), _ptr(s), k,
                          _ptr(base_f32), _ptr(base_i64) if n_i else None, _ptr(out_f32),
                          _ptr(out_i64f) if n_i else None, *args_tail)
            else:
                _lib.call("plato_agg_fedavg_deltas", _ptr(ptr_f32), ptr_i, _ptr(w), _ptr(s), k,
                          _ptr(out_f32), _ptr(out_i64f) if n_i else None, *args_tail)
        else:
            _lib.tune_call("plato_agg_tune_fedavg", self.variant, int(base_f32 is not None), _ptr(ptr_f32),
                      ptr_i, _ptr(w), _ptr(s), k, _ptr(base_f32),
                      _ptr(base_i64) if n_i else None, _ptr(out_f32),
                      _ptr(out_i64f) if n_i else None, *args_tail)

    # ------------------------------------------------------ host-facing API
    def begin(self, template: Mapping[str, torch.Tensor], capacity: int,
              codec: str = "native") -> "AggregationRound":
        """Start a round: device arenas for up to ``capacity`` client payloads.

        ``template`` is the baseline (its keys, shapes, dtypes define the arena);
        ``codec`` is how the client payloads arrive ("native" or "bf16").
        """
        if capacity <= 0:
            raise ValueError("no client payloads to aggregate")
        layout = self._prepare(template, capacity, codec)
        # The previous round's kernel may still read the slab / baseline arena:
        # order this round's H2D copies (copy stream) after it.
        self._copy_stream.wait_stream(torch.cuda.current_stream(self.device))
        return AggregationRound(self, layout, capacity, codec)

    def stage_clients(self, payloads: Sequence[Mapping[str, torch.Tensor]], template=None,
                      what: str = "weights_received") -> ArenaLayout:
        """Pack and copy K CPU payloads into the client slab (rows 0..K-1)."""
        template = template if template is not None else payloads[0]
        layout = self._prepare(template, len(payloads))
        for i, sd in enumerate(payloads):
            layout.check_compatible(sd, f"{what}[{i}]")
            self._stager.put(sd, self._slab.f32[i], self._slab.i64[i])
        return layout

    def aggregate_weights(self, baseline: Mapping[str, torch.Tensor],
                          weights_received: Sequence[Mapping[str, torch.Tensor]],
                          weights: Sequence[float], scales: Sequence[float] | None = None
                          ) -> "OrderedDict[str, torch.Tensor]":
        """``update_weights(aggregate_deltas(compute_weight_deltas(b, X)))`` on the GPU.

        Returns CPU tensors in baseline key order: fp32 for every entry (int64
        entries come back as fp32 ``float(b) + avg`` exactly like the
        reference's ``update_weights``; ``load_weights`` truncates them).
        """
        k = len(weights_received)
        if k == 0:
            raise ValueError("no client payloads to aggregate")
        if len(weights) != k:
            raise ValueError("weights must have one entry per client")
        rnd = self.begin(baseline, k, payload_codec(weights_received[0]))
        rnd.put_baseline(baseline)
        for i, sd in enumerate(weights_received):
            rnd.put_client(i, sd)
        rnd.launch(weights, scales)
        return rnd.result()

    def aggregate_deltas(self, deltas_received: Sequence[Mapping[str, torch.Tensor]],
                         weights: Sequence[float], scales: Sequence[float] | None = None
                         ) -> "OrderedDict[str, torch.Tensor]":
        """``Server.aggregate_deltas`` on the GPU: ``avg = sum_i delta_i * w_i`` (fp32)."""
        k = len(deltas_received)
        if k == 0:
            raise ValueError("no client deltas to aggregate")
        if len(weights) != k:
            raise ValueError("weights must have one entry per client")
        rnd = self.begin(deltas_received[0], k)
        for i, sd in enumerate(deltas_received):
            rnd.put_client(i, sd, what="deltas_received")
        rnd.launch(weights, scales, deltas=True)
        return rnd.result()

    def weighted_sum(self, tensors: Sequence, weights: Sequence[float]) -> torch.Tensor:
        """``avg = trainer.zeros(n); avg += t_i * w_i`` over same-size vectors, in order.

        fp32 tensors follow torch's fp32 chain (one deltas-mode launch, fp32
        result).  float64 numpy vectors follow the reference's numpy promotion
        — the plaintext half of HE hybrid FedAvg (plato/servers/fedavg_he.py:
        88-98), whose vectors come from ``np.append`` into float64 arrays
        (plato/utils/homo_enc.py:50-63): ``avg += unenc_w * w`` falls back to
        numpy and the accumulator becomes float64, so the sum runs in float64
        (``plato_agg_weighted_sum_f64``) and the result is a float64 tensor.
        """
        if len(tensors) == 0:
            raise ValueError("no tensors to sum")
        if len(weights) != len(tensors):
            raise ValueError("weights must have one entry per vector")
        first = tensors[0]
        if (isinstance(first, np.ndarray) and first.dtype == np.float64) or \
                (isinstance(first, torch.Tensor) and first.dtype == torch.float64):
            return self._weighted_sum_f64(tensors, weights)
        sds = [OrderedDict(v=torch.as_tensor(t)) for t in tensors]
        return self.aggregate_deltas(sds, weights)["v"]

    def _weighted_sum_f64(self, vectors, weights) -> torch.Tensor:
        """float64 vectors: ``((0 + x_0*w_0) + x_1*w_1) + ...`` in float64 (``plato_agg_weighted_sum_f64``)."""
        n = int(np.asarray(vectors[0]).size)
        host = torch.empty((len(vectors), max(2, -(-n // 2) * 2)), dtype=torch.float64, pin_memory=True)
        for r, v in enumerate(vectors):
            v = torch.as_tensor(np.asarray(v, dtype=np.float64)).reshape(-1)
            if v.numel() != n:
                raise ValueError("vectors must have the same length")
            host[r, :n].copy_(v)
        dev = host.to(self.device, non_blocking=True)
        w = torch.tensor([float(x) for x in weights], dtype=torch.float64).to(self.device)
        ptrs = torch.tensor([dev.data_ptr() + r * dev.stride(0) * 8 for r in range(len(vectors))],
                            dtype=torch.int64).to(self.device)
        out = torch.empty(max(2, n), dtype=torch.float64, device=self.device)
        stream = torch.cuda.current_stream(self.device)
        _lib.call("plato_agg_weighted_sum_f64", _ptr(ptrs), _ptr(w), len(vectors), _ptr(out), n,
                  _stream_handle(stream))
        return out[:n].cpu()

    def compute_weight_deltas(self, baseline: Mapping[str, torch.Tensor],
                              weights_received: Sequence[Mapping[str, torch.Tensor]]
                              ) -> list["OrderedDict[str, torch.Tensor]"]:
        """``Algorithm.compute_weight_deltas`` (``algorithms/fedavg.py:13-27``) on the GPU.

        int64 entries keep int64 deltas, as ``current - baseline`` does.
        """
        k = len(weights_received)
        if k == 0:
            return []
        layout = self.stage_clients(weights_received, template=baseline)
        self._stager.put(baseline, self._base.f32, self._base.i64)
        stream = torch.cuda.current_stream(self.device)
        self._stager.fence(stream)
        h = _stream_handle(stream)
        out = []
        for i in range(k):
            df = torch.empty(layout.row_f32, dtype=torch.float32, device=self.device)
            di = torch.empty(layout.row_i64, dtype=torch.int64, device=self.device)
            _lib.call("plato_agg_compute_deltas", _ptr(self._slab.f32[i]), _ptr(self._slab.i64[i]),
                      _ptr(self._base.f32), _ptr(self._base.i64), _ptr(df), _ptr(di),
                      layout.n_f32, layout.n_i64, h)
            out.append(layout.unpack(df[: layout.n_f32].to("cpu"), di[: layout.n_i64].to("cpu")))
        return out

    def update_weights(self, baseline: Mapping[str, torch.Tensor],
                       deltas: Mapping[str, torch.Tensor]) -> "OrderedDict[str, torch.Tensor]":
        """``Algorithm.update_weights`` (``algorithms/fedavg.py:29-37``): ``b + avg`` in fp32."""
        layout = self._prepare(baseline, 1)
        # avg is fp32 for every key (trainers/basic.py:63); stage it as a
        # float32 row for both regions.
        avg_f = torch.empty(layout.row_f32, dtype=torch.float32, device=self.device)
        avg_i = torch.empty(layout.row_i64, dtype=torch.float32, device=self.device)
        f32 = [deltas[e.name].reshape(-1).to(torch.float32) for e in layout.entries if e.region == F32]
        i64 = [deltas[e.name].reshape(-1).to(torch.float32) for e in layout.entries if e.region == I64]
        if f32:
            avg_f[: layout.n_f32].copy_(torch.cat(f32))
        if i64:
            avg_i[: layout.n_i64].copy_(torch.cat(i64))
        self._stager.put(baseline, self._base.f32, self._base.i64)
        stream = torch.cuda.current_stream(self.device)
        self._stager.fence(stream)
        out_f = torch.empty_like(avg_f)
        out_i = torch.empty_like(avg_i)
        _lib.call("plato_agg_update_weights", _ptr(self._base.f32), _ptr(self._base.i64), _ptr(avg_f),
                  _ptr(avg_i), _ptr(out_f), _ptr(out_i), layout.n_f32, layout.n_i64,
                  _stream_handle(stream))
        return layout.unpack(out_f[: layout.n_f32].to("cpu"), out_i[: layout.n_i64].to("cpu"))

    def mix_weights(self, baseline: Mapping[str, torch.Tensor],
                    received: Mapping[str, torch.Tensor], mixing: float
                    ) -> "OrderedDict[str, torch.Tensor]":
        """FedAsync: ``b * (1 - m) + x * m`` (``fedasync_algorithm.py:15-18``)."""
        layout = self.stage_clients([received], template=baseline)
        self._stager.put(baseline, self._base.f32, self._base.i64)
        stream = torch.cuda.current_stream(self.device)
        self._stager.fence(stream)
        one_minus = float(np.float32(1 - mixing))
        m = float(np.float32(mixing))
        out_f = torch.empty(layout.row_f32, dtype=torch.float32, device=self.device)
        out_i = torch.empty(layout.row_i64, dtype=torch.float32, device=self.device)
        _lib.call("plato_agg_mix_weights", _ptr(self._slab.f32[0]), _ptr(self._slab.i64[0]),
                  _ptr(self._base.f32), _ptr(self._base.i64), one_minus, m, _ptr(out_f),
                  _ptr(out_i), layout.n_f32, layout.n_i64, _stream_handle(stream))
        return layout.unpack(out_f[: layout.n_f32].to("cpu"), out_i[: layout.n_i64].to("cpu"))


class _KernelTimer:
    """HIP events on ``stream`` around the launches of a ``with`` block; the round's ``timings[name + "_ms"]``
    is filled once the stream has passed them (``AggregationRound._resolve_timers``, after the method's sync)."""

    def __init__(self, rnd: "AggregationRound", name: str, stream):
        self.rnd, self.name, self.stream = rnd, name, stream

    def __enter__(self):
        self.e0 = torch.cuda.Event(enable_timing=True)
        self.e0.record(self.stream)
        return self

    def __exit__(self, *exc):
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record(self.stream)
        self.rnd._timers.append((self.name, self.e0, e1))
        return False


class AggregationRound(RobustLaunches, VariantLaunches):
    """One aggregation: client rows staged H2D (in any order), then one launch: the FedAvg sums here, the
    robust aggregators in ``plato_amd.robust``, the variant servers' reductions in ``plato_amd.reductions``.
    Every launch over staged rows starts from :meth:`_staged_rows`.

    Rows are slots; the summation order is given at :meth:`launch` time by
    ``order`` (default: slot order), matching ``self.updates`` order in the
    reference regardless of the order payloads arrived in.
    """

    deltas = False  # (set per round in __init__; decoded rounds hold decoded weights)

    def __init__(self, engine: FedAvgEngine, layout: ArenaLayout, capacity: int, codec: str = "native"):
        self.engine = engine
        self.layout = layout
        self.capacity = capacity
        self.codec = codec
        self.slab = engine._slabs[codec]
        self.stager = engine._stagers[codec]
        self.staged = [False] * capacity
        # per slot: device pointers of its fp32 / int64 rows (round slab or an arrival slot)
        self._pf = [0] * capacity
        self._pi = [0] * capacity
        self._rows: list = [None] * capacity  # per slot: (slab, row) that holds it (fetch_rows)
        # QSGD codec: per slot max_v per entry (layout order) and the clients' quantization level
        self._mv: list = [None] * capacity
        self._level: int | None = None
        self.has_baseline = False
        self.event: torch.cuda.Event | None = None
        self._out = None
        self._t0 = time.perf_counter()
        self._kernel_events = None
        self.timings: dict = {}
        self._k = 0
        self._decoded = None
        self._timers: list = []
        # Delta arenas: every staged slot is turned into x - b in place on the copy stream as it is staged
        # (compute_weight_deltas, plato/algorithms/fedavg.py:13-27, the same fp32 differences and int64
        # wrapping differences the kernels would form), so the reductions that re-read the baseline per
        # client (FedAdp's dots) stream no baseline.  The kernels then run in their deltas forms and the
        # final update adds the baseline once (plato_agg_update_weights: b + acc, the fused epilogue's sum).
        self.deltas = bool(getattr(engine, "delta_arenas", False)) and codec == "native"
        self._converted: set = set()
        self._robust = False           # set by the robust launches: no baseline, every entry comes back fp32
        self._base_key = None          # baseline_key of the staged baseline
        self._arrival_base_ok = None   # the device check of the arrival baseline, once per round

    def _to_delta(self, slot: int) -> None:
        """Turn staged slot ``slot`` into its delta x - b, in place, on the copy stream (after its H2D)."""
        if not self.has_baseline:
            raise ValueError("delta arenas: stage the baseline before the clients")
        key = (self._pf[slot], self._pi[slot])
        if key in self._converted:
            return
        self.engine._to_delta(*key, self._base, self.stager.stream)
        self._converted.add(key)

    def _raw_only(self, what: str) -> None:
        if self.deltas:
            raise ValueError(f"{what} reads the clients' weights; this round holds deltas (engine.delta_arenas)")

    def _timed(self, name: str, stream) -> _KernelTimer:
        return _KernelTimer(self, name, stream)

    def _resolve_timers(self) -> None:
        """Device times of the timed launches (call after the stream has been synchronised)."""
        for name, e0, e1 in self._timers:
            self.timings[name + "_ms"] = e0.elapsed_time(e1)
        self._timers = []

    @property
    def _base(self) -> DeviceArena:
        """The baseline arena this round's kernels read (the engine's; a decoded round has its own)."""
        return self.engine._base

    def put_baseline(self, baseline: Mapping[str, torch.Tensor]) -> None:
        self.layout.check_compatible(baseline, "baseline_weights")
        eng = self.engine
        if self.deltas and any(self.staged):
            raise ValueError("delta arenas: the clients were staged as deltas of the previous baseline")
        eng._stager.put(baseline, eng._base.f32, eng._base.i64)
        self.has_baseline = True
        self._base_key = baseline_key(baseline)
        self._arrival_base_ok = None
        self._decoded = None

    def put_client(self, slot: int, payload: Mapping[str, torch.Tensor],
                   what: str = "weights_received") -> None:
        if not 0 <= slot < self.capacity:
            raise IndexError(f"slot {slot} outside [0, {self.capacity})")
        self.layout.check_compatible(payload, f"{what}[{slot}]", self.codec)
        self._coded_scales(slot, payload)
        if self.deltas and not self.has_baseline:
            raise ValueError("delta arenas: stage the baseline before the clients")
        self.stager.put(payload, self.slab.f32[slot], self.slab.i64[slot])
        pf, pi = self.slab.row_pointers([slot])
        self._pf[slot], self._pi[slot] = int(pf[0]), int(pi[0])
        self._rows[slot] = (self.slab, slot)
        self._converted.discard((self._pf[slot], self._pi[slot]))  # fresh weights in the row
        if self.deltas:
            self._to_delta(slot)  # behind this client's H2D on the copy stream
        self.staged[slot] = True
        self._decoded = None  # decoded rows are per staged set

    def _coded_scales(self, slot: int, payload) -> None:
        if self.codec != "qsgd":
            return
        level = int(payload.level)
        if self._level is not None and level != self._level:
            raise ValueError(f"QSGD payloads of one round must share quantization_level ({level} != {self._level})")
        self._level = level
        self._mv[slot] = payload.max_v_array(self.layout.keys())

    def adopt(self, slot: int, payload: Mapping[str, torch.Tensor]) -> bool:
        """Use ``payload``'s copy already staged at arrival (``FedAvgEngine.prestage``), if any.  Returns False
        (nothing done) when there is none this round may use; the caller then stages it with put_client."""
        if not 0 <= slot < self.capacity:
            raise IndexError(f"slot {slot} outside [0, {self.capacity})")
        rec = self.engine._arrivals.lookup(payload, self.codec, self.layout.signature)
        if rec is None:
            return False
        how = adopt_rule(rec.delta_key, self.deltas, self.has_baseline, self._base_key, self._arrival_base_matches)
        if how is Adopt.REFUSE:
            return False  # a delta against another model (or a weight round): stage the payload again
        self._coded_scales(slot, payload)
        self._pf[slot], self._pi[slot] = rec.rows
        self._rows[slot] = rec.slot
        if how is Adopt.AS_FORMED:
            self._converted.add(rec.rows)  # turned into its delta at arrival, against this round's baseline
        elif self.deltas:  # the arrival row holds the weights: its delta now, in place (the row is this round's)
            self._to_delta(slot)
        self.staged[slot] = True
        self._decoded = None  # decoded rows are per staged set
        return True

    def _arrival_base_matches(self) -> bool:
        """The model the arrivals were turned into deltas against has this round's baseline bits
        (``arrivals.adopt_rule``'s ``same_bits``): the two staged arenas compared once per round on the
        device, after both copies (copy stream).  A mismatch makes the round stage its arrivals again."""
        if self._arrival_base_ok is None:
            eng, lay = self.engine, self.layout
            arr = eng._arrival_base
            if arr is None or arr.layout.signature != lay.signature:
                self._arrival_base_ok = False
            else:
                torch.cuda.current_stream(eng.device).wait_stream(eng._copy_stream)
                self._arrival_base_ok = (
                    same_f32_bits(self._base.f32[: lay.n_f32], arr.f32[: lay.n_f32], lay.f32_padding(eng.device))
                    and torch.equal(self._base.i64[: lay.n_i64], arr.i64[: lay.n_i64]))
        return self._arrival_base_ok

    def launch(self, weights: Sequence[float], scales: Sequence[float] | None = None,
               order: Sequence[int] | None = None, deltas: bool = False) -> None:
        """Enqueue the fused kernel (stream-ordered after every staged copy)."""
        order = list(range(len(weights))) if order is None else list(order)
        if len(order) != len(weights):
            raise ValueError("order and weights must have the same length")
        self._staged(order)
        if not deltas and not self.has_baseline:
            raise ValueError("baseline not staged")
        if deltas and self.codec != "native":
            raise ValueError("deltas are fp32 (x - b promotes coded payloads); use the native codec")
        eng = self.engine
        lay = self.layout
        self.timings["stage_ms"] = (time.perf_counter() - self._t0) * 1e3
        self._k = len(order)
        w, s = eng._upload_weights(weights, scales)
        pf = np.asarray([self._pf[i] for i in order], dtype=np.int64)
        pi = np.asarray([self._pi[i] for i in order], dtype=np.int64)
        tf, ti = eng._pointer_tables(pf, pi)
        stream = torch.cuda.current_stream(eng.device)
        self.stager.fence(stream)
        out_f = torch.empty(lay.row_f32, dtype=torch.float32, device=eng.device)
        out_i = torch.empty(lay.row_i64, dtype=torch.float32, device=eng.device)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        if self.codec == "qsgd":
            n_i = lay.n_i64
            mv = torch.from_numpy(np.ascontiguousarray(np.stack([self._mv[i] for i in order], axis=1))).to(eng.device)
            cf, ci = eng._chunks(lay, eng.QSGD_CHUNK)
            ncf, nci = int(cf.shape[0]), int(ci.shape[0])
            args = (_ptr(tf), _ptr(ti) if n_i else None, len(order), _ptr(mv), len(lay.entries),
                    float(self._level - 1), _ptr(w), _ptr(s), _ptr(cf), ncf, _ptr(ci) if nci else None, nci,
                    _ptr(self._base.f32), _ptr(self._base.i64) if n_i else None, _ptr(out_f),
                    _ptr(out_i) if n_i else None, lay.n_f32, n_i, _stream_handle(stream))
            if eng.qsgd_variant is None:
                _lib.call("plato_agg_fedavg_qsgd", *args)
            else:  # tuning / tests
                _lib.tune_call("plato_agg_tune_fedavg_qsgd", eng.qsgd_variant, *args)
            w = (w, mv)
        elif self.codec == "bf16":
            n_i = lay.n_i64
            _lib.call("plato_agg_fedavg_weights_bf16", _ptr(tf), _ptr(ti) if n_i else None, _ptr(w), _ptr(s),
                      len(order), _ptr(self._base.f32), _ptr(self._base.i64) if n_i else None, _ptr(out_f),
                      _ptr(out_i) if n_i else None, lay.n_f32, n_i, _stream_handle(stream))
        elif self.deltas and not deltas:  # delta arenas: acc = sum_i d_i * w_i, then b + acc
            acc_f = torch.empty_like(out_f)
            acc_i = torch.empty_like(out_i)
            eng.launch_fedavg(lay, tf, ti, w, s, len(order), None, None, acc_f, acc_i, stream)
            n_i = lay.n_i64
            _lib.call("plato_agg_update_weights", _ptr(self._base.f32), _ptr(self._base.i64) if n_i else None,
                      _ptr(acc_f), _ptr(acc_i) if n_i else None, _ptr(out_f), _ptr(out_i) if n_i else None,
                      lay.n_f32, n_i, _stream_handle(stream))
            w = (w, acc_f, acc_i)
        else:
            eng.launch_fedavg(lay, tf, ti, w, s, len(order), None if deltas else self._base.f32,
                              None if deltas else self._base.i64, out_f, out_i, stream)
        e1.record(stream)
        self._kernel_events = (e0, e1)
        self._fetch(stream, out_f, out_i, (tf, ti, w, s))

    def launch_w64(self, weights64: Sequence[float], weights_i64: Sequence[float] | None = None,
                   order: Sequence[int] | None = None, deltas: bool = False) -> None:
        """FedAvg with float64 weights on the fp32 entries (``plato_agg_fedavg_w64``).

        ``acc = fp32(double(acc) + double(d) * w64[i])`` for fp32 entries,
        ``acc += fp32(fp32(d) * fp32(w_i64[i]))`` for int64 entries (default:
        ``w_i64 = weights64``): the RL server's float64 smart weighting
        (rl_server.py:66-71) and HE's float64 plaintext vectors (fedavg_he.py:88-98).
        """
        order = list(range(len(weights64))) if order is None else list(order)
        if len(order) != len(weights64):
            raise ValueError("order and weights must have the same length")
        _, tf, ti, stream = self._staged_rows(order, baseline=not deltas, raw=None if deltas else "launch_w64")
        eng = self.engine
        self.timings["stage_ms"] = (time.perf_counter() - self._t0) * 1e3
        self._k = len(order)
        w64 = torch.from_numpy(np.asarray([float(w) for w in weights64], dtype=np.float64)).to(eng.device)
        wi = fp32_weights(weights64 if weights_i64 is None else weights_i64)
        if len(wi) != len(order):
            raise ValueError("weights_i64 must have one entry per client")
        wi = torch.from_numpy(wi).to(eng.device)
        out_f, out_i = self._out_rows()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        _lib.call("plato_agg_fedavg_w64", *self._regions(tf, ti), _ptr(w64), _ptr(wi), len(order),
                  *self._baseline(deltas), *self._regions(out_f, out_i), *self._sizes(stream))
        e1.record(stream)
        self._kernel_events = (e0, e1)
        self._fetch(stream, out_f, out_i, (tf, ti, w64, wi))

    def _fetch(self, stream, out_f: torch.Tensor, out_i: torch.Tensor, keep=()) -> None:
        """D2H into pooled pinned buffers, stream-ordered; result() only waits."""
        lay = self.layout
        host_f, host_i = self.engine._result_pool(lay).get()
        host_f.copy_(out_f[: lay.n_f32], non_blocking=True)
        host_i.copy_(out_i[: lay.n_i64], non_blocking=True)
        self.event = torch.cuda.Event(enable_timing=True)
        self.event.record(stream)
        # keep device buffers alive until the copies finish
        self._out = (host_f, host_i, out_f, out_i, keep)

    def _staged(self, slots: Sequence[int]) -> list[int]:
        return staged_slots(self.capacity, self.staged, slots)

    def _check_slots(self, slots: Sequence[int]) -> list[int]:
        slots = self._staged(slots)
        if not slots:
            raise ValueError("no client slots")
        if self.codec != "native":
            raise ValueError("per-entry kernels take fp32 rows: run them on rnd.decoded() for coded payloads")
        return slots

    def _staged_rows(self, slots: Sequence[int], *, baseline: bool = True, raw: str | None = None,
                     tables: bool = True):
        """What a launch over staged rows starts from: (slots, fp32 pointer table, int64 pointer table,
        stream), the stream ordered behind the staged copies.  Refuses slots that are not staged or hold
        codes, a missing baseline where the launch reads one (``baseline``), and a round of deltas where
        ``raw`` names a launch that reads the weights.  ``tables=False`` (a launch that packs the row
        pointers into a table of its own) uploads none and returns ``None`` for both."""
        slots = self._check_slots(slots)
        if baseline and not self.has_baseline:
            raise ValueError("baseline not staged")
        if raw is not None:
            self._raw_only(raw)
        tf, ti = self._row_tables(slots) if tables else (None, None)
        stream = torch.cuda.current_stream(self.engine.device)
        self.stager.fence(stream)
        return slots, tf, ti, stream

    def _row_tables(self, slots: Sequence[int]):
        return self.engine._pointer_tables(np.asarray([self._pf[i] for i in slots], dtype=np.int64),
                                           np.asarray([self._pi[i] for i in slots], dtype=np.int64))

    def _out_rows(self):
        lay, dev = self.layout, self.engine.device
        return (torch.empty(lay.row_f32, dtype=torch.float32, device=dev),
                torch.empty(lay.row_i64, dtype=torch.float32, device=dev))

    def _regions(self, f32: torch.Tensor, i64: torch.Tensor):
        """The C-ABI arguments of a two-region buffer: NULL for the int64 half of a layout without one."""
        return f32.data_ptr(), (i64.data_ptr() if self.layout.n_i64 else None)

    def _baseline(self, deltas: bool):
        """The C-ABI arguments of the baseline; (NULL, NULL) where the rows already hold x - b (``deltas``:
        the kernels then run in their deltas forms and read none)."""
        return (None, None) if deltas else self._regions(self._base.f32, self._base.i64)

    def _sizes(self, stream):  # the tail of a kernel call
        return self.layout.n_f32, self.layout.n_i64, stream.cuda_stream

    def stage_reference(self, state_dict: Mapping[str, torch.Tensor]) -> DeviceArena:
        """Port's stored global model as a device arena, staged ahead of :meth:`model_similarities`
        (which otherwise stages it itself: a PCIe copy of the whole model on the similarity's path)."""
        return self._stage_model(state_dict, "reference model", torch.cuda.current_stream(self.engine.device))

    def _stage_model(self, state_dict, what: str, stream) -> DeviceArena:
        """A native model (e.g. Port's stored global model) as a device arena of this round's layout."""
        self.layout.check_compatible(state_dict, what)
        eng = self.engine
        arena = DeviceArena(self.layout, eng.device)
        eng._stager.put(state_dict, arena.f32, arena.i64)
        eng._stager.fence(stream)
        return arena

    def decoded(self) -> "AggregationRound":
        """This round as the reference's server sees coded payloads: every entry float32.

        The reference dequantizes in its inbound processor (plato/processors/
        model_dequantize.py:15-18, model_dequantize_qsgd.py:34-60) before any
        server code runs, so FedAtt / FedAdp / Polaris / Port reduce float32
        state_dicts whose num_batches_tracked counters are float32 too.  The
        staged slots (bf16 or QSGD codes in HBM) and the baseline are decoded
        once by ``plato_agg_decode_rows`` into fp32 rows of ``layout.promoted()``
        (the counters become fp32 entries, the baseline's cast with RNE), and
        the returned round runs the per-entry kernels on them.  Slots are the
        same; the plain FedAvg launch stays on this round (decode in registers).
        A native round returns itself.
        """
        if self.codec == "native":
            return self
        if self._decoded is not None:
            return self._decoded
        if not self.has_baseline:
            raise ValueError("baseline not staged")
        eng, lay = self.engine, self.layout
        slots = [i for i in range(self.capacity) if self.staged[i]]
        if not slots:
            raise ValueError("no client slots staged")
        play = lay.promoted()
        rnd = _DecodedRound(self, play, slots)
        stream = torch.cuda.current_stream(eng.device)
        self.stager.fence(stream)
        eng._stager.fence(stream)
        cf, ci = eng._chunks(lay, 4096)
        ncf, nci = int(cf.shape[0]), int(ci.shape[0])
        dst_off = lay.row_f32
        h = _stream_handle(stream)

        def decode(codec, src_f, src_i, dsts, mv=None, divisor=0.0):
            k = len(dsts)
            tab = torch.from_numpy(np.asarray(list(src_f) + list(src_i) + list(dsts), dtype=np.int64)).to(eng.device)
            _lib.call("plato_agg_decode_rows", _lib.PLATO_AGG_DECODE[codec], tab.data_ptr(), tab.data_ptr() + 8 * k, k,
                      _ptr(mv), float(divisor), _ptr(cf), ncf, _ptr(ci) if nci else None, nci, dst_off,
                      tab.data_ptr() + 16 * k, h)
            return tab

        keep = [decode("native", [_ptr(eng._base.f32)], [_ptr(eng._base.i64)], [_ptr(rnd._own_base.f32)])]
        rows = rnd.slab.row_pointers(range(len(slots)))[0]
        mv = None
        if self.codec == "qsgd":
            mv = torch.from_numpy(np.ascontiguousarray(np.stack([self._mv[i] for i in slots], axis=1))).to(eng.device)
        keep.append(decode(self.codec, [self._pf[i] for i in slots], [self._pi[i] for i in slots], list(rows), mv,
                           0.0 if self._level is None else float(self._level - 1)))
        rnd._keep_decode = (keep, mv)
        self._decoded = rnd
        return rnd

    def ready(self) -> bool:
        return self.event is not None and self.event.query()

    def wait(self) -> None:
        """Block until the result is in host memory (releases the GIL: safe on a worker thread)."""
        if self.event is None:
            raise RuntimeError("launch() first")
        self.event.synchronize()

    def algorithmic_bytes(self) -> int:
        """HBM bytes of the launch: K client arenas + baseline read, result written."""
        if self._robust:  # no baseline; the counters come back as fp32
            lay = self.layout
            return (self._k + 1) * lay.n_f32_data * 4 + self._k * lay.n_i64 * 8 + lay.n_i64 * 4
        return self.layout.algorithmic_bytes(self._k)

    def result(self) -> "OrderedDict[str, torch.Tensor]":
        if self.event is None:
            raise RuntimeError("launch() first")
        self.event.synchronize()
        if self._kernel_events is not None:
            e0, e1 = self._kernel_events
            self.timings["kernel_ms"] = e0.elapsed_time(e1)
            self.timings["d2h_ms"] = e1.elapsed_time(self.event)
        self.timings["total_ms"] = (time.perf_counter() - self._t0) * 1e3
        self._resolve_timers()  # launches timed with _timed and fetched by this call (launch_robust)
        host_f, host_i = self._out[0], self._out[1]
        self._out = None
        return self.layout.unpack(host_f, host_i)


class _DecodedRound(AggregationRound):
    """A coded round's slots and baseline as fp32 rows of the promoted layout (AggregationRound.decoded)."""

    def __init__(self, parent: AggregationRound, layout: ArenaLayout, slots: Sequence[int]):
        eng = parent.engine
        self._parent = parent
        self.engine = eng
        self.layout = layout
        self.capacity = parent.capacity
        self.codec = "native"
        self.slab = ClientSlab(layout, len(slots), eng.device)
        self.stager = parent.stager
        self.staged = [False] * parent.capacity
        self._pf = [0] * parent.capacity
        self._pi = [0] * parent.capacity
        self._rows = [None] * parent.capacity
        rows = self.slab.row_pointers(range(len(slots)))
        for r, slot in enumerate(slots):
            self._pf[slot], self._pi[slot] = int(rows[0][r]), int(rows[1][r])
            self._rows[slot] = (self.slab, r)
            self.staged[slot] = True
        self._mv = [None] * parent.capacity
        self._level = None
        self.has_baseline = True
        self._base_key = self._arrival_base_ok = None
        self._robust = False
        self.event = None
        self._out = None
        self._t0 = parent._t0
        self._kernel_events = None
        self.timings = {}
        self._timers = []
        self._k = 0
        self._decoded = None
        self._own_base = DeviceArena(layout, eng.device)

    @property
    def _base(self) -> DeviceArena:
        return self._own_base

    def decoded(self) -> "AggregationRound":
        return self

    def _stage_model(self, state_dict, what: str, stream) -> DeviceArena:
        # staged in the model's own layout, then promoted like the baseline (counters cast to fp32)
        native = AggregationRound._stage_model(self._parent, state_dict, what, stream)
        out = DeviceArena(self.layout, self.engine.device)
        lay = self._parent.layout
        cf, ci = self.engine._chunks(lay, 4096)
        ncf, nci = int(cf.shape[0]), int(ci.shape[0])
        tab = torch.tensor([native.f32.data_ptr(), native.i64.data_ptr(), out.f32.data_ptr()], dtype=torch.int64,
                           device=self.engine.device)
        _lib.call("plato_agg_decode_rows", _lib.PLATO_AGG_DECODE["native"], tab.data_ptr(), tab.data_ptr() + 8, 1,
                  None, 0.0, _ptr(cf), ncf, _ptr(ci) if nci else None, nci, lay.row_f32, tab.data_ptr() + 16,
                  _stream_handle(stream))
        self._keep_model = (native, tab)
        return out


def cast_to_int64(src_f32: torch.Tensor, stream: torch.cuda.Stream | None = None) -> torch.Tensor:
    """load_state_dict's fp32 -> int64 truncating copy, on the device."""
    if not src_f32.is_cuda or src_f32.dtype != torch.float32:
        raise ValueError("cast_to_int64 expects a CUDA float32 tensor")
    src = src_f32.contiguous()
    dst = torch.empty(src.shape, dtype=torch.int64, device=src.device)
    stream = stream or torch.cuda.current_stream(src.device)
    _lib.call("plato_agg_cast_f32_i64", _ptr(src), _ptr(dst), src.numel(), _stream_handle(stream))
    return dst
