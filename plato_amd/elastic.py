"""Elastic sub-model aggregation: the depth- and width-heterogeneous server of the reference's model-search
examples (examples/model_search/sysheterofl: ``Algorithm.aggregation``, the "ElasticArch" search).

Every client trains a sub-model that differs from the global one in depth (whole keys are missing from its
payload) and in width per stage; its tensors are leading-corner boxes of the global model's, a 4-D one on
all four dims.  With G the global ``state_dict`` and the clients' in arrival order, for every key of G in
G's order (the normative text is in include/plato_agg.h, DESIGN.md §23 has the design):

* the key has a rank from ``G[key].dim()`` (:func:`rank_of`): 4, 2 and 1 are their own rank, any other dim
  is rank 0, and so is a 1-D running statistic with ``update_track=False``;
* a client takes part in a key of rank >= 1 that its payload holds, with the box ``[:s0, ...]`` of its own
  shape.  Per element, in fp32: ``acc = g``; ``acc = acc + x_k`` over the clients that hold the key and
  cover the element, in arrival order; ``out = (acc - g) / max(count, 1)`` (``plato_agg_elastic_mean``);
* every result is float32.  An integer key of G whose dim is not 1, 2 or 4 (the 0-D ``num_batches_tracked``
  counters) gives float32 zeros, written here without GPU work; any other key that is not float32 is refused.

The tables of :func:`build_tables` are pure numpy; :class:`ElasticRound` stages and launches.  Not built:
integer entries of rank >= 1, several GPUs, bf16 and QSGD payloads.
"""

from __future__ import annotations

import time
from collections import OrderedDict
from typing import Mapping, Sequence

import numpy as np
import torch

from . import _lib
from .arena import ArenaLayout, payload_codec
from .submodel import ROW_ALIGN, _State, _numel

MAX_K = _lib.PLATO_AGG_ELASTIC_MAX_K
TILE = _lib.PLATO_AGG_ELASTIC_TILE
ENTRY_WORDS = _lib.PLATO_AGG_ELASTIC_ENTRY_WORDS
BOX_WORDS = _lib.PLATO_AGG_ELASTIC_BOX_WORDS
_INTEGER = (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)


def rank_of(name: str, dim: int, update_track: bool = True) -> int:
    """The number of leading dims a client's box is cut on: ``dim`` itself for 4, 2 and 1, else 0; a 1-D
    running statistic is left alone (rank 0) with ``update_track=False``."""
    dim = int(dim)
    if dim not in (4, 2, 1):
        return 0
    if dim == 1 and not update_track and ("running" in name or "tracked" in name):
        return 0
    return dim


def global_layout(global_model: Mapping[str, torch.Tensor]) -> tuple[ArenaLayout, list]:
    """(the float32 entries of the global model packed back to back in its key order, the names of the
    integer entries that become float32 zeros on the host).  Refuses every other entry."""
    spec, zeros = [], []
    for name, tensor in global_model.items():
        if not isinstance(tensor, torch.Tensor):
            raise ValueError(f"global model[{name!r}] is {type(tensor)}, not a tensor")
        if tensor.dtype == torch.float32:
            spec.append((name, tuple(tensor.shape), "f32"))
        elif tensor.dtype in _INTEGER and tensor.dim() not in (1, 2, 4):
            zeros.append(name)
        else:
            raise ValueError(f"global model[{name!r}] is {tensor.dtype} with {tensor.dim()} dims; elastic aggregation "
                             "takes torch.float32 entries, and integer entries whose dim is not 1, 2 or 4")
    return ArenaLayout.from_shapes(spec), zeros


def client_signature(glayout: ArenaLayout, payload: Mapping[str, torch.Tensor], update_track: bool,
                     what: str) -> tuple:
    """``((name, shape), ...)`` of the entries of ``payload`` the aggregation reads (held, rank >= 1), in the
    global layout's order.  Refuses a tensor that is not float32, one with another number of dims and an
    extent above the global's; keys that the global model lacks are ignored."""
    sig = []
    for e in glayout.entries:
        if e.name not in payload or not rank_of(e.name, len(e.shape), update_track):
            continue
        t = payload[e.name]
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise ValueError(f"{what}[{e.name!r}] is {getattr(t, 'dtype', type(t))}, expected torch.float32")
        client_box(e.shape, [[d] for d in range(len(e.shape))], tuple(t.shape), f"{what}[{e.name!r}]")
        sig.append((e.name, tuple(t.shape)))
    return tuple(sig)


def compact_layout(signature: tuple) -> ArenaLayout:
    """A client's held entries of rank >= 1 packed back to back: its row."""
    return ArenaLayout.from_shapes([(name, shape, "f32") for name, shape in signature])


def canonical_view(shape: tuple, rank: int, holders: Sequence[tuple]) -> tuple[tuple, list]:
    """``([A, B, C, D], groups)`` of an entry of ``shape`` and rank ``rank`` whose holders have the shapes
    ``holders``.  ``groups`` lists the entry's dims per view dim, right-aligned (the leading view dims are 1).
    A trailing dim in which every holder has the full extent is merged into the dim before it; rank 0, or no
    holder, is one run ``[1, 1, 1, numel]``."""
    if not rank or not holders:
        return (1, 1, 1, _numel(shape)), [list(range(len(shape)))]
    groups = [[d] for d in range(rank)]
    while len(groups) > 1 and all(h[groups[-1][0]] == shape[groups[-1][0]] for h in holders):
        tail = groups.pop()
        groups[-1] += tail
    view = tuple(_numel(shape[d] for d in g) for g in groups)
    return (1,) * (4 - len(view)) + view, groups


def client_box(gshape: tuple, groups: list, cshape: tuple, what: str) -> tuple:
    """(a, b, c, d) of a client tensor of ``cshape`` in the view of the global entry that ``groups`` gives
    (:func:`canonical_view`)."""
    if len(cshape) != len(gshape):
        raise ValueError(f"{what} has {len(cshape)} dims, the global entry {len(gshape)}")
    if any(c > g for c, g in zip(cshape, gshape)):
        raise ValueError(f"{what} is {tuple(cshape)}: an extent above the global's {tuple(gshape)}")
    box = tuple(int(cshape[g[0]]) * _numel(gshape[d] for d in g[1:]) for g in groups)
    return (1,) * (4 - len(box)) + box


class ElasticTables:
    """The host tables of one ``plato_agg_elastic_mean`` call (include/plato_agg.h)."""

    def __init__(self, entries: np.ndarray, boxes: np.ndarray, row_len: np.ndarray, n_out: int):
        self.entries, self.boxes, self.row_len, self.n_out = entries, boxes, row_len, n_out

    @property
    def k(self) -> int:
        return int(self.row_len.shape[0])

    def covered(self) -> int:
        """Client elements the kernel reads: the sum of the boxes."""
        b = self.boxes
        return int((b[:, 0] * b[:, 1] * b[:, 2] * b[:, 3]).sum())  # every box is below 2^38 elements

    def absent_share(self) -> float:
        """The share of (entry, client) pairs without a box: what the compact list leaves out."""
        pairs = len(self.entries) * self.k
        return 1.0 - len(self.boxes) / pairs if pairs else 0.0

    def algorithmic_bytes(self) -> int:
        """The global region read and the result written once, every covered client element read once."""
        return 4 * (2 * self.n_out + self.covered())


def build_tables(glayout: ArenaLayout, signatures: Sequence[tuple], update_track: bool = True) -> ElasticTables:
    """The entry table [entries, 8], the compact box table [boxes, 6] and the row lengths for K clients
    given by their shape signatures (:func:`client_signature`), in arrival order."""
    layouts = {sig: compact_layout(sig) for sig in set(signatures)}
    held = [layouts[sig] for sig in signatures]
    ents = glayout.entries
    entries = np.zeros((len(ents), ENTRY_WORDS), dtype=np.int64)
    boxes = []
    tile0 = 0
    for idx, e in enumerate(ents):
        rank = rank_of(e.name, len(e.shape), update_track)
        holders = [(c, lay[e.name]) for c, lay in enumerate(held) if e.name in lay._by_name] if rank else []
        view, groups = canonical_view(e.shape, rank, [ce.shape for _, ce in holders])
        entries[idx] = (e.offset, *view, tile0, len(boxes), len(holders))
        tile0 += -(-e.numel // TILE)
        for c, ce in holders:  # by ascending client: the arrival order is the order of the sum
            boxes.append((*client_box(e.shape, groups, ce.shape, f"client {c}[{e.name!r}]"), ce.offset, c))
    row_len = np.asarray([lay.n_f32 for lay in held], dtype=np.int64)
    return ElasticTables(entries, np.asarray(boxes, dtype=np.int64).reshape(-1, BOX_WORDS), row_len, glayout.n_f32)


def check_payloads(payloads: Sequence[Mapping[str, torch.Tensor]]) -> None:
    """The refusals that need no model: no payloads, too many, coded payloads."""
    if len(payloads) == 0:
        raise ValueError("no client payloads to aggregate")
    if len(payloads) > MAX_K:
        raise ValueError(f"elastic aggregation takes at most {MAX_K} clients, got {len(payloads)}")
    for i, p in enumerate(payloads):
        codec = payload_codec(p)
        if codec != "native":
            raise ValueError(f"elastic aggregation takes native payloads; weights_received[{i}] holds {codec} codes")


class ElasticRound:
    """One elastic aggregation on a ``FedAvgEngine``: every refusal in the constructor (no GPU work), then
    :meth:`stage` (pinned packs and H2D copies on the copy stream), :meth:`launch`, :meth:`result`."""

    def __init__(self, engine, global_model: Mapping[str, torch.Tensor],
                 payloads: Sequence[Mapping[str, torch.Tensor]], update_track: bool = True):
        if getattr(engine, "primary", None) is not None:
            raise NotImplementedError("elastic aggregation runs on one GPU: use FedAvgEngine")
        check_payloads(payloads)
        self.engine, self.update_track = engine, bool(update_track)
        self.global_model, self.payloads = global_model, list(payloads)
        self.glayout, self.zeros = global_layout(global_model)
        self.signatures = [client_signature(self.glayout, p, self.update_track, f"weights_received[{i}]")
                           for i, p in enumerate(self.payloads)]
        self.tables = build_tables(self.glayout, self.signatures, self.update_track)
        self.timings: dict = {}
        self._timers: list = []
        self._t0 = time.perf_counter()
        self.event = None
        self._out = None
        self._keep = None

    # ---------------------------------------------------------------- staging
    def _state(self) -> _State:
        st = getattr(self.engine, "_elastic", None)
        if st is None:
            st = self.engine._elastic = _State()
        return st

    def _stager(self, st: _State, layout: ArenaLayout):
        from .engine import _Stager

        hit = st.stagers.get(layout.signature)
        if hit is None:
            hit = st.stagers[layout.signature] = _Stager(layout, self.engine.device, depth=2,
                                                         stream=self.engine._copy_stream)
        return hit

    def stage(self) -> None:
        """The global model's float32 entries and every client's row to HBM: one pinned pack and one copy
        each, on the engine's copy stream.  Clients of one shape signature share a layout and a stager."""
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
        nbytes = _lib.lib().plato_agg_elastic_tables_bytes(len(tab.entries), len(tab.boxes))
        d_tables = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        # pinned: the call's copies of the tables are stream-ordered, and the round keeps them until result()
        h_entries = torch.from_numpy(tab.entries).pin_memory()
        h_boxes = torch.from_numpy(tab.boxes).pin_memory() if len(tab.boxes) else None
        with self._timed("elastic_mean", stream):
            _lib.call("plato_agg_elastic_mean", st.global_dev.data_ptr(), rows.data_ptr(), tab.k,
                      tab.row_len.ctypes.data, h_entries.data_ptr(), len(tab.entries),
                      h_boxes.data_ptr() if h_boxes is not None else None, len(tab.boxes),
                      d_tables.data_ptr(), out.data_ptr(), n, stream.cuda_stream)
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
        """CPU float32 tensors in the global model's key order: the float32 entries from the device, the
        integer counters as zeros of their shape."""
        self.wait()
        self._resolve_timers()
        self.timings["kernel_ms"] = self.timings.get("elastic_mean_ms")
        self.timings["total_ms"] = (time.perf_counter() - self._t0) * 1e3
        host, self._out, self._keep = self._out, None, None
        mine = self.glayout.unpack(host, None)
        out = OrderedDict()
        for name, tensor in self.global_model.items():
            out[name] = mine[name] if name in mine else torch.zeros(tensor.shape, dtype=torch.float32)
        return out


class ElasticAggregates:
    """``aggregate_elastic`` over CPU payloads (mixin of ``FedAvgEngine``)."""

    def begin_elastic(self, global_model: Mapping[str, torch.Tensor],
                      payloads: Sequence[Mapping[str, torch.Tensor]], update_track: bool = True) -> ElasticRound:
        """A checked round (every refusal is raised here, before anything is staged)."""
        return ElasticRound(self, global_model, payloads, update_track)

    def aggregate_elastic(self, global_model: Mapping[str, torch.Tensor],
                          payloads: Sequence[Mapping[str, torch.Tensor]], update_track: bool = True
                          ) -> "OrderedDict[str, torch.Tensor]":
        """``Algorithm.aggregation`` of the reference's sysheterofl example on the GPU: every element of
        ``global_model`` becomes the mean of the clients that hold its key and whose leading-corner box covers
        it, summed on top of the global value in arrival order and with it subtracted again, as the reference
        does.  Returns CPU float32 tensors in the global model's key order."""
        rnd = self.begin_elastic(global_model, payloads, update_track)
        rnd.stage()
        rnd.launch()
        return rnd.result()
