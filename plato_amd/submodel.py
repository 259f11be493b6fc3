"""Sub-model aggregation: the width-heterogeneous servers of the reference's model-search examples
(examples/model_search/{heterofl,fjord,fedrolex,anycostfl}: ``Algorithm.aggregation``).

Every client trains a sub-model whose tensors are leading-corner boxes ``value[:s0, :s1, ...]`` of the
global model's; the server averages every global element over the clients whose box covers it.  With G
the global ``state_dict`` and the clients' in arrival order, for every key of G in G's order:

* a key that contains neither ``"weight"`` nor ``"bias"`` *passes through*: the result is a copy of
  ``G[key]`` (dtype and shape kept); the clients' values are never read and may be absent;
* any other key *participates* with a prefix rank r (:func:`prefix_rank`): client k's tensor has shape
  ``(s_0 .. s_{r-1}, G's trailing dims)`` and covers the elements whose first r indices are below them.
  Per element, in fp32: ``acc = g``; ``acc = acc + x_k`` over the covering clients in arrival order;
  ``out = (acc - g) / max(count, 1)`` (``plato_agg_submodel_mean``).  With r = 0 no client covers the
  entry and its clients' values are never read either.

The tables of :func:`build_tables` are pure numpy; :class:`SubmodelRound` stages and launches.  Out of
scope: ``sysheterofl`` (boxes on four dims, keys missing per client, int64 counters divided as floats: it
is ``plato_amd.elastic``, with an entry point and a table format of its own; its tables and its round are
the classes here, :class:`_BoxTables` and :class:`_BoxRound`, with what differs filled in), several GPUs,
bf16 and QSGD payloads, and rows prestaged at arrival (sub-model payloads are staged here).
"""

from __future__ import annotations

import time
from collections import OrderedDict
from typing import Mapping, Sequence

import numpy as np
import torch

from . import _lib
from .arena import ArenaLayout, payload_codec

#: ``G[key].dim()`` -> prefix rank, per rule; any other dim has rank 0
RULES = {
    "heterofl": {4: 2, 2: 2, 1: 1},              # HeteroFL, FjORD
    "fedrolex": {4: 2, 2: 2, 1: 1, 3: 3},        # FedRolex, AnyCostFL
}
MAX_K = _lib.PLATO_AGG_SUBMODEL_MAX_K
TILE = _lib.PLATO_AGG_SUBMODEL_TILE
ABSENT = _lib.PLATO_AGG_SUBMODEL_ABSENT
ROW_ALIGN = 64  # client rows start 256-byte aligned in the slab


def participates(name: str) -> bool:
    return "weight" in name or "bias" in name


def prefix_rank(rule: str, name: str, dim: int) -> int | None:
    """The prefix rank of entry ``name`` with ``dim`` dims under ``rule``; None: the entry passes through."""
    if rule not in RULES:
        raise ValueError(f"unknown sub-model rule {rule!r} (supported: {sorted(RULES)})")
    if not participates(name):
        return None
    return RULES[rule].get(int(dim), 0)


def _numel(shape) -> int:
    n = 1
    for d in shape:
        n *= int(d)
    return n


def global_layout(global_model: Mapping[str, torch.Tensor]) -> ArenaLayout:
    """The participating entries of the global model, packed back to back in its key order."""
    spec = []
    for name, tensor in global_model.items():
        if not participates(name):
            continue
        if not isinstance(tensor, torch.Tensor) or tensor.dtype != torch.float32:
            raise ValueError(f"global model[{name!r}] is {getattr(tensor, 'dtype', type(tensor))}; "
                             "participating entries are torch.float32")
        spec.append((name, tuple(tensor.shape), "f32"))
    return ArenaLayout.from_shapes(spec)


def client_signature(glayout: ArenaLayout, rule: str, payload: Mapping[str, torch.Tensor], what: str) -> tuple:
    """``((name, shape), ...)`` of the entries of ``payload`` the aggregation reads (rank >= 1), in the
    global layout's order.  Refuses a missing key and a tensor that is not float32."""
    sig = []
    for e in glayout.entries:
        if not prefix_rank(rule, e.name, len(e.shape)):
            continue
        if e.name not in payload:
            raise ValueError(f"{what} is missing {e.name!r}")
        t = payload[e.name]
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise ValueError(f"{what}[{e.name!r}] is {getattr(t, 'dtype', type(t))}, expected torch.float32")
        sig.append((e.name, tuple(t.shape)))
    return tuple(sig)


def compact_layout(signature: tuple) -> ArenaLayout:
    """A client's entries that the aggregation reads, packed back to back: its row."""
    return ArenaLayout.from_shapes([(name, shape, "f32") for name, shape in signature])


def canonical_view(shape: tuple, rank: int) -> tuple[int, int, int]:
    """[P, Q, L] of an entry of ``shape`` with prefix rank ``rank`` (0: one run no client covers)."""
    if rank == 1:
        return 1, 1, int(shape[0])
    if rank == 2:
        return int(shape[0]), 1, _numel(shape[1:])
    if rank == 3:
        return int(shape[0]), int(shape[1]), int(shape[2])
    return 1, 1, _numel(shape)


def client_box(gshape: tuple, rank: int, cshape: tuple, what: str) -> tuple[int, int, int]:
    """(p, q, l) of a client tensor of ``cshape`` in the canonical view of the global entry."""
    if len(cshape) != len(gshape):
        raise ValueError(f"{what} has {len(cshape)} dims, the global entry {len(gshape)}")
    if tuple(cshape[rank:]) != tuple(gshape[rank:]):
        raise ValueError(f"{what} is {tuple(cshape)}: its trailing dims differ from the global's {tuple(gshape)}")
    for c, g in zip(cshape[:rank], gshape[:rank]):
        if c > g:
            raise ValueError(f"{what} is {tuple(cshape)}: an extent above the global's {tuple(gshape)}")
    if rank == 1:
        return 1, 1, int(cshape[0])
    if rank == 2:
        return int(cshape[0]), 1, int(cshape[1]) * _numel(gshape[2:])
    return int(cshape[0]), int(cshape[1]), int(cshape[2])


class _BoxTables:
    """The host tables of one call (include/plato_agg.h); a box row begins with its ``EXTENTS`` extents."""

    EXTENTS: int

    def __init__(self, entries: np.ndarray, boxes: np.ndarray, row_len: np.ndarray, n_out: int):
        self.entries, self.boxes, self.row_len, self.n_out = entries, boxes, row_len, n_out

    @property
    def k(self) -> int:
        return int(self.row_len.shape[0])

    def covered(self) -> int:
        """Client elements the kernel reads: the sum of the boxes."""
        return int(self.boxes[..., :self.EXTENTS].prod(axis=-1).sum())  # every box is below 2^38 elements

    def algorithmic_bytes(self) -> int:
        """The global region read and the result written once, every covered client element read once."""
        return 4 * (2 * self.n_out + self.covered())


class SubmodelTables(_BoxTables):
    """The host tables of one ``plato_agg_submodel_mean`` call: boxes [entries, K, 4]."""

    EXTENTS = 3


def build_tables(glayout: ArenaLayout, signatures: Sequence[tuple], rule: str) -> SubmodelTables:
    """The entry table, the box table [entries, K, 4] and the row lengths for K clients given by their
    shape signatures (:func:`client_signature`), in arrival order."""
    if rule not in RULES:
        raise ValueError(f"unknown sub-model rule {rule!r} (supported: {sorted(RULES)})")
    k = len(signatures)
    layouts = {sig: compact_layout(sig) for sig in set(signatures)}
    ents = glayout.entries
    entries = np.zeros((len(ents), _lib.PLATO_AGG_SUBMODEL_ENTRY_WORDS), dtype=np.int64)
    boxes = np.zeros((len(ents), k, _lib.PLATO_AGG_SUBMODEL_BOX_WORDS), dtype=np.int64)
    boxes[..., 3] = ABSENT
    tile0 = 0
    for idx, e in enumerate(ents):
        rank = prefix_rank(rule, e.name, len(e.shape))
        P, Q, L = canonical_view(e.shape, rank)
        entries[idx] = (e.offset, P, Q, L, tile0, 0)
        tile0 += -(-e.numel // TILE)
        if not rank:
            continue
        for c, sig in enumerate(signatures):
            ce = layouts[sig][e.name]
            boxes[idx, c] = (*client_box(e.shape, rank, ce.shape, f"client {c}[{e.name!r}]"), ce.offset)
    row_len = np.asarray([layouts[sig].n_f32 for sig in signatures], dtype=np.int64)
    return SubmodelTables(entries, boxes, row_len, glayout.n_f32)


def check_payloads(payloads: Sequence[Mapping[str, torch.Tensor]], rule: str) -> None:
    """The refusals that need no model: an unknown rule, no payloads, too many, coded payloads."""
    if rule not in RULES:
        raise ValueError(f"unknown sub-model rule {rule!r} (supported: {sorted(RULES)})")
    if len(payloads) == 0:
        raise ValueError("no client payloads to aggregate")
    if len(payloads) > MAX_K:
        raise ValueError(f"sub-model aggregation takes at most {MAX_K} clients, got {len(payloads)}")
    for i, p in enumerate(payloads):
        codec = payload_codec(p)
        if codec != "native":
            raise ValueError(f"sub-model aggregation takes native payloads; weights_received[{i}] holds {codec} codes")


class _State:
    """What an engine keeps across sub-model rounds: compact layouts and their stagers per signature,
    the client slab and the global arena."""

    def __init__(self):
        self.layouts: dict = {}
        self.globals: dict = {}
        self.stagers: dict = {}
        self.slab: torch.Tensor | None = None
        self.global_dev: torch.Tensor | None = None


class _BoxRound:
    """One aggregation of leading-corner boxes on a ``FedAvgEngine``: every refusal in the constructor (no
    GPU work), then :meth:`stage` (pinned packs and H2D copies on the copy stream), :meth:`launch`,
    :meth:`result`.  A kind (:class:`SubmodelRound`, ``plato_amd.elastic.ElasticRound``) gives KIND for the
    messages, SLOT (the engine attribute that keeps its :class:`_State`: a slab and stagers per kind) and
    KERNEL for the timings; ``_check()``, the other refusals, returning (global layout, signatures, tables);
    ``_tables_bytes()`` and ``_mean(...)``, the library calls over ``self.tables`` (pointers as integers,
    ``h_boxes`` None without boxes); and ``_absent(tensor)``, the result for a key the device did not produce."""

    def __init__(self, engine, global_model: Mapping[str, torch.Tensor],
                 payloads: Sequence[Mapping[str, torch.Tensor]]):
        if getattr(engine, "primary", None) is not None:
            raise NotImplementedError(f"{self.KIND} aggregation runs on one GPU: use FedAvgEngine")
        self.engine, self.global_model, self.payloads = engine, global_model, list(payloads)
        self.glayout, self.signatures, self.tables = self._check()
        self.timings: dict = {}
        self._timers: list = []
        self._t0 = time.perf_counter()
        self.event = None
        self._out = None
        self._keep = None

    # ---------------------------------------------------------------- staging
    def _state(self) -> _State:
        st = getattr(self.engine, self.SLOT, None)
        if st is None:
            st = _State()
            setattr(self.engine, self.SLOT, st)
        return st

    def _stager(self, st: _State, layout: ArenaLayout):
        from .engine import _Stager

        hit = st.stagers.get(layout.signature)
        if hit is None:
            hit = st.stagers[layout.signature] = _Stager(layout, self.engine.device, depth=2,
                                                         stream=self.engine._copy_stream)
        return hit

    def stage(self) -> None:
        """The global model's entries on the device and every client's row to HBM: one pinned pack and one
        copy each, on the engine's copy stream.  Clients of one shape signature share a layout and a stager."""
        eng, st, dev = self.engine, self._state(), self.engine.device
        if eng._copy_stream is None:
            eng._copy_stream = torch.cuda.Stream(dev)
        # an earlier round's kernel may still read the slab and the global arena
        eng._copy_stream.wait_stream(torch.cuda.current_stream(dev))
        self.glayout = st.globals.setdefault(self.glayout.signature, self.glayout)  # keeps its result pool
        n = self.glayout.n_f32
        if st.global_dev is None or st.global_dev.numel() < max(n, 1):
            st.global_dev = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
        if n:
            self._stager(st, self.glayout).put(self.global_model, st.global_dev, None)
        offsets, at = [], 0
        for sig in self.signatures:
            if sig not in st.layouts:
                st.layouts[sig] = compact_layout(sig)
            offsets.append(at)
            at += -(-st.layouts[sig].n_f32 // ROW_ALIGN) * ROW_ALIGN
        if st.slab is None or st.slab.numel() < max(at, 1):
            st.slab = torch.empty(max(at, 1), dtype=torch.float32, device=dev)
        for off, sig, payload in zip(offsets, self.signatures, self.payloads):
            lay = st.layouts[sig]
            if lay.n_f32:
                self._stager(st, lay).put(payload, st.slab[off:off + lay.n_f32], None)
        self._row_ptrs = np.asarray([st.slab.data_ptr() + 4 * off for off in offsets], dtype=np.int64)
        self.timings["stage_ms"] = (time.perf_counter() - self._t0) * 1e3

    # ----------------------------------------------------------------- launch
    def _timed(self, name: str, stream):
        from .engine import _KernelTimer

        return _KernelTimer(self, name, stream)

    def launch(self) -> None:
        eng, st, dev, tab = self.engine, self._state(), self.engine.device, self.tables
        stream = torch.cuda.current_stream(dev)
        stream.wait_stream(eng._copy_stream)
        n = tab.n_out
        out = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
        rows = torch.from_numpy(self._row_ptrs).to(dev)
        d_tables = torch.empty(self._tables_bytes(), dtype=torch.uint8, device=dev)
        # pinned: the call's copies of the tables are stream-ordered, and the round keeps them until result()
        h_entries = torch.from_numpy(tab.entries).pin_memory()
        h_boxes = torch.from_numpy(tab.boxes).pin_memory() if tab.boxes.size else None
        with self._timed(self.KERNEL, stream):
            self._mean(st.global_dev.data_ptr(), rows.data_ptr(), h_entries.data_ptr(),
                       h_boxes.data_ptr() if h_boxes is not None else None, d_tables.data_ptr(), out.data_ptr(),
                       stream.cuda_stream)
        host = eng._result_pool(self.glayout).get()[0]
        host.copy_(out[:n], non_blocking=True)
        self.event = torch.cuda.Event(enable_timing=True)
        self.event.record(stream)
        self._out = host
        self._keep = (out, rows, d_tables, h_entries, h_boxes)

    def _resolve_timers(self) -> None:
        for name, e0, e1 in self._timers:
            self.timings[name + "_ms"] = e0.elapsed_time(e1)
        self._timers = []

    def wait(self) -> None:
        if self.event is None:
            raise RuntimeError("launch() first")
        self.event.synchronize()

    def algorithmic_bytes(self) -> int:
        return self.tables.algorithmic_bytes()

    def result(self) -> "OrderedDict[str, torch.Tensor]":
        """CPU tensors in the global model's key order: the entries on the device float32 from there, the
        others as :meth:`_absent` gives them."""
        self.wait()
        self._resolve_timers()
        self.timings["kernel_ms"] = self.timings.get(self.KERNEL + "_ms")
        self.timings["total_ms"] = (time.perf_counter() - self._t0) * 1e3
        host, self._out, self._keep = self._out, None, None
        mine = self.glayout.unpack(host, None)
        out = OrderedDict()
        for name, tensor in self.global_model.items():
            out[name] = mine[name] if name in mine else self._absent(tensor)
        return out


class SubmodelRound(_BoxRound):
    """One sub-model aggregation (:class:`_BoxRound`); an entry that passes through is a clone of the
    global model's."""

    KIND, SLOT, KERNEL = "sub-model", "_submodel", "submodel_mean"

    def __init__(self, engine, global_model: Mapping[str, torch.Tensor],
                 payloads: Sequence[Mapping[str, torch.Tensor]], rule: str = "heterofl"):
        self.rule = rule
        super().__init__(engine, global_model, payloads)

    def _check(self) -> tuple:
        check_payloads(self.payloads, self.rule)
        glayout = global_layout(self.global_model)
        signatures = [client_signature(glayout, self.rule, p, f"weights_received[{i}]")
                      for i, p in enumerate(self.payloads)]
        return glayout, signatures, build_tables(glayout, signatures, self.rule)

    def _tables_bytes(self) -> int:
        return _lib.lib().plato_agg_submodel_tables_bytes(self.tables.k, len(self.tables.entries))

    def _mean(self, d_global, d_rows, h_entries, h_boxes, d_tables, d_out, stream) -> None:
        tab = self.tables
        _lib.call("plato_agg_submodel_mean", d_global, d_rows, tab.k, tab.row_len.ctypes.data, h_entries, h_boxes,
                  len(tab.entries), d_tables, d_out, tab.n_out, stream)

    def _absent(self, tensor: torch.Tensor) -> torch.Tensor:
        return tensor.detach().clone()


class SubmodelAggregates:
    """``aggregate_submodels`` over CPU payloads (mixin of ``FedAvgEngine``)."""

    def begin_submodels(self, global_model: Mapping[str, torch.Tensor],
                        payloads: Sequence[Mapping[str, torch.Tensor]], rule: str = "heterofl") -> SubmodelRound:
        """A checked round (every refusal is raised here, before anything is staged)."""
        return SubmodelRound(self, global_model, payloads, rule)

    def aggregate_submodels(self, global_model: Mapping[str, torch.Tensor],
                            payloads: Sequence[Mapping[str, torch.Tensor]], rule: str = "heterofl"
                            ) -> "OrderedDict[str, torch.Tensor]":
        """``Algorithm.aggregation`` of the reference's HeteroFL and FjORD (``rule="heterofl"``) or FedRolex
        and AnyCostFL (``rule="fedrolex"``) on the GPU: every element of a participating entry of
        ``global_model`` becomes the mean of the clients whose leading-corner box covers it, summed on top
        of the global value in arrival order and with it subtracted again, as the reference does.  Returns
        CPU tensors in the global model's key order; entries that pass through are clones of its own."""
        rnd = self.begin_submodels(global_model, payloads, rule)
        rnd.stage()
        rnd.launch()
        return rnd.result()
