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

from collections import OrderedDict
from typing import Mapping, Sequence

import numpy as np
import torch

from . import _lib
from .arena import ArenaLayout, payload_codec
from .submodel import ROW_ALIGN, _BoxRound, _BoxTables, _numel, compact_layout  # noqa: F401  (this module's too)

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


class ElasticTables(_BoxTables):
    """The host tables of one ``plato_agg_elastic_mean`` call: the compact box list [boxes, 6]."""

    EXTENTS = 4

    def absent_share(self) -> float:
        """The share of (entry, client) pairs without a box: what the compact list leaves out."""
        pairs = len(self.entries) * self.k
        return 1.0 - len(self.boxes) / pairs if pairs else 0.0


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


class ElasticRound(_BoxRound):
    """One elastic aggregation (``plato_amd.submodel._BoxRound``); every result is float32, an integer
    counter zeros of its shape."""

    KIND, SLOT, KERNEL = "elastic", "_elastic", "elastic_mean"

    def __init__(self, engine, global_model: Mapping[str, torch.Tensor],
                 payloads: Sequence[Mapping[str, torch.Tensor]], update_track: bool = True):
        self.update_track = bool(update_track)
        super().__init__(engine, global_model, payloads)

    def _check(self) -> tuple:
        check_payloads(self.payloads)
        glayout, self.zeros = global_layout(self.global_model)
        signatures = [client_signature(glayout, p, self.update_track, f"weights_received[{i}]")
                      for i, p in enumerate(self.payloads)]
        return glayout, signatures, build_tables(glayout, signatures, self.update_track)

    def _tables_bytes(self) -> int:
        return _lib.lib().plato_agg_elastic_tables_bytes(len(self.tables.entries), len(self.tables.boxes))

    def _mean(self, d_global, d_rows, h_entries, h_boxes, d_tables, d_out, stream) -> None:
        tab = self.tables
        _lib.call("plato_agg_elastic_mean", d_global, d_rows, tab.k, tab.row_len.ctypes.data, h_entries,
                  len(tab.entries), h_boxes, len(tab.boxes), d_tables, d_out, tab.n_out, stream)

    def _absent(self, tensor: torch.Tensor) -> torch.Tensor:
        return torch.zeros(tensor.shape, dtype=torch.float32)


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
