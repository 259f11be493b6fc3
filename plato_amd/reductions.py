"""The variant servers' reductions over a round's staged rows: FedAtt's per-entry norms and entrywise sum,
FedAdp's dots, Polaris' squared deltas and Port's cosine similarities, each in the reference's own float32
order.  :class:`VariantLaunches` is a mixin of ``engine.AggregationRound``, which holds what every launch
starts from (``_staged_rows``, ``_baseline``, ``_regions``); the baseline is reached through ``self._base``
only (a decoded round has its own).
"""

from __future__ import annotations

from typing import Mapping, Sequence

import numpy as np
import torch

from . import _lib
from .arena import F32, DeviceArena, fedadp_order


def entrywise_weights(weights, n_entries: int, k: int) -> np.ndarray:
    """``weights`` as the contiguous ``[entries, clients]`` fp32 array ``plato_agg_fedavg_entrywise`` takes,
    rounded to fp32 like torch's scalar multiply."""
    w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).astype(np.float32))
    if w.shape != (n_entries, k):
        raise ValueError(f"weights must be [entries={n_entries}, clients={k}], got {w.shape}")
    return w


def _flat_stride(n_flat: int) -> int:
    """Floats per row of a buffer of flat vectors (64-aligned rows)."""
    return max(64, -(-n_flat // 64) * 64)


class VariantLaunches:
    """The per-entry and flattened-model reductions (mixin of ``AggregationRound``)."""

    def entry_stats(self, slots: Sequence[int], v: tuple | None = None, deltas: bool = False):
        """Per (client, entry) fp64 sums over the staged slots (``plato_agg_entry_stats``).

        ``d_i = x_i - baseline`` (``deltas=False``) or ``x_i``.  ``v`` is an
        optional device vector ``(fp32 arena, fp32 values of the int64
        entries)``, e.g. :meth:`launch_entrywise`'s ``device=True`` output.
        Returns ``(dv [K, E] | None, dd [K, E], vv [E] | None)`` as float64
        numpy arrays, entries in layout order.
        """
        deltas = deltas or self.deltas  # delta arenas: the rows are the deltas
        slots, tf, ti, stream = self._staged_rows(slots, baseline=not deltas)
        eng, lay = self.engine, self.layout
        k, n_e = len(slots), len(lay.entries)
        cf, ci = eng._chunks(lay, eng.STATS_CHUNK)
        ncf, nci = int(cf.shape[0]), int(ci.shape[0])
        ws = torch.empty((eng.lib.plato_agg_entry_stats_workspace(k, ncf + nci) + 7) // 8,
                         dtype=torch.float64, device=eng.device)
        out = torch.empty((2 * k + 1) * n_e, dtype=torch.float64, device=eng.device)
        vf, vi = (None, None) if v is None else v
        _lib.call("plato_agg_entry_stats", *self._regions(tf, ti), k, *self._baseline(deltas),
                  None if vf is None else vf.data_ptr(), vi.data_ptr() if (vi is not None and lay.n_i64) else None,
                  cf.data_ptr(), ncf, ci.data_ptr() if nci else None, nci, n_e, lay.n_f32, lay.n_i64, ws.data_ptr(),
                  out.data_ptr(), stream.cuda_stream)
        res = out.cpu().numpy().reshape(2 * k + 1, n_e)
        if v is None:
            return None, res[k:2 * k].copy(), None
        return res[:k].copy(), res[k:2 * k].copy(), res[2 * k].copy()

    def entry_norms(self, slots: Sequence[int]) -> np.ndarray:
        """fp32 ``torch.linalg.norm`` of each (client, entry) delta in torch's CPU order.

        Bit-equal to the reference's ``torch.linalg.norm(-delta)``
        (fedatt_algorithm.py:39), by ``plato_agg_entry_norms_f32``; with
        ``FedAvgEngine.norms_long_threshold`` set, the long fp32 entries go to
        ``plato_agg_port_norms`` on a side stream instead (measured slower, off
        by default).  Returns ``[E, K]`` float32 (entries in layout order,
        clients in ``slots`` order).
        """
        slots, tf, ti, stream = self._staged_rows(slots, raw="entry_norms")
        eng, lay = self.engine, self.layout
        k, n_e = len(slots), len(lay.entries)
        ei = eng._norm_tables(lay)[1]
        out = torch.zeros(k * n_e, dtype=torch.float32, device=eng.device)
        ef, keep = self._long_norms_aside(slots, out, stream)
        nef, nei = int(ef.shape[0]), int(ei.shape[0])
        if nef or nei:
            with self._timed("entry_norms", stream):
                _lib.call("plato_agg_entry_norms_f32", *self._regions(tf, ti), k, *self._baseline(False),
                          ef.data_ptr() if nef else None, nef, ei.data_ptr() if nei else None, nei, n_e,
                          lay.n_f32, lay.n_i64, out.data_ptr(), stream.cuda_stream)
        if keep:
            stream.wait_stream(eng.side_stream())
        res = np.ascontiguousarray(out.cpu().numpy().reshape(k, n_e).T)
        self._resolve_timers()
        del keep
        return res

    def _long_norms_aside(self, slots: Sequence[int], out: torch.Tensor, stream):
        """``FedAvgEngine.norms_long_threshold``: the norms of the fp32 entries at least that long, by
        ``plato_agg_port_norms`` on the side stream (started here; the caller joins it after its own launch)
        and scattered into ``out``.  Returns the fp32 norm table (one piece per entry, longest first) of the
        entries left to ``plato_agg_entry_norms_f32`` and the device buffers to keep until ``out`` is read;
        with the option off (the default) that is every entry and nothing."""
        eng, lay = self.engine, self.layout
        long_ids = [] if eng.norms_long_threshold is None else sorted(
            (i for i, e in enumerate(lay.entries) if e.region == F32 and e.numel >= eng.norms_long_threshold),
            key=lambda i: -lay.entries[i].numel)
        if not long_ids:
            return eng._norm_tables(lay)[0], ()
        k, n_e = len(slots), len(lay.entries)
        side = eng.side_stream()  # the long chains first, on their own stream
        side.wait_stream(stream)
        base_f = self._base.f32.data_ptr()
        xs = [self._pf[j] + 4 * lay.entries[e].offset for e in long_ids for j in slots]
        bs = [base_f + 4 * lay.entries[e].offset for e in long_ids for _ in slots]
        lens = np.asarray([lay.entries[e].numel for e in long_ids for _ in slots], dtype=np.uint32)
        n_max = int(lens.max())
        tab = np.asarray(xs + xs + bs + bs, dtype=np.int64)  # int64 tables unused (one fp32 segment)
        seg = np.zeros(1, dtype=[("flat", "<u8"), ("src", "<u8"), ("numel", "<u8"), ("region", "<u4"),
                                 ("flags", "<u4")])
        seg["numel"] = n_max
        v = len(xs)
        with torch.cuda.stream(side):
            dt = torch.from_numpy(tab).to(eng.device)
            dl = torch.from_numpy(lens.view(np.int32)).to(eng.device)
            ds = torch.from_numpy(seg.view(np.int64).copy()).to(eng.device)
            dn = torch.empty(v, dtype=torch.float32, device=eng.device)
            p8, n8 = dt.data_ptr(), 8 * v
            _lib.call("plato_agg_port_norms", p8, p8 + n8, p8 + 2 * n8, p8 + 3 * n8, v, dl.data_ptr(), ds.data_ptr(),
                      1, n_max, lay.n_f32, 0, dn.data_ptr(), None, side.cuda_stream)
            # scatter: vector (li, j) -> out[j * n_e + entry]
            idx = torch.from_numpy(np.asarray([j * n_e + e for e in long_ids for j in range(k)],
                                              dtype=np.int64)).to(eng.device)
            out.index_copy_(0, idx, dn)
        return eng._norm_tables_without(lay, tuple(long_ids)), (dt, dl, ds, dn, idx)

    def launch_entrywise(self, weights: np.ndarray, order: Sequence[int] | None = None, scale: float = 1.0,
                         noise: Mapping[str, torch.Tensor] | None = None, noise_scale: float = 0.0,
                         add_base: bool = True, deltas: bool = False, device: bool = False):
        """Weighted sum with a weight per (entry, client) (``plato_agg_fedavg_entrywise``).

        ``weights`` is ``[E, K]`` (entries in layout order, clients in
        ``order``), rounded to fp32 like torch's scalar multiply.  ``noise``
        is a state_dict of fp32 tensors added as ``noise * noise_scale``.
        ``device=True`` returns the device result ``(fp32 arena, int64
        entries as fp32)`` instead of scheduling the D2H for :meth:`result`.
        """
        order = range(np.shape(weights)[1]) if order is None else order
        slots, tf, ti, stream = self._staged_rows(
            order, baseline=not deltas, raw="launch_entrywise(add_base=True)" if add_base and not deltas else None)
        deltas = deltas or self.deltas  # delta arenas: the staged rows are the deltas the kernel would form
        if deltas and add_base:
            raise ValueError("add_base needs the baseline (deltas=False)")
        eng, lay = self.engine, self.layout
        k, n_e = len(slots), len(lay.entries)
        dw = torch.from_numpy(entrywise_weights(weights, n_e, k)).to(eng.device)
        cf, ci = eng._chunks(lay, eng.ENTRYWISE_CHUNK)
        nz = None
        if noise is not None:
            nz = DeviceArena(lay, eng.device, i64_dtype=torch.float32)
            lay.check_compatible(noise, "noise", "f32")
            nst = eng._f32_stager(lay)
            nst.put(noise, nz.f32, nz.i64)
            nst.fence(stream)
        out_f, out_i = self._out_rows()
        ncf, nci = int(cf.shape[0]), int(ci.shape[0])
        _lib.call("plato_agg_fedavg_entrywise", *self._regions(tf, ti), k, dw.data_ptr(), n_e,
                  cf.data_ptr(), ncf, ci.data_ptr() if nci else None, nci, *self._baseline(deltas),
                  *((None, None) if nz is None else self._regions(nz.f32, nz.i64)),
                  float(scale), float(noise_scale), _lib.PLATO_AGG_ADD_BASE if add_base else 0,
                  *self._regions(out_f, out_i), *self._sizes(stream))
        if device:
            # inputs stay referenced by the caller's stream order; nothing to fetch
            self._keep = (tf, ti, dw, nz)
            return out_f, out_i
        self._fetch(stream, out_f, out_i, (tf, ti, dw, nz))
        return None

    # ------------------------------------------- flattened-model reductions
    def _flat_segments(self, order: Sequence[int], neg_div_after_first: bool) -> torch.Tensor:
        """plato_agg_segment rows for the layout's entries in ``order`` (device, cached)."""
        lay, eng = self.layout, self.engine
        key = ("flat_segments", tuple(order), neg_div_after_first, str(eng.device))
        hit = lay._cache.get(key)
        if hit is None:
            rows = np.zeros((len(order), 4), dtype=np.uint64)
            flat = 0
            for j, idx in enumerate(order):
                e = lay.entries[idx]
                flags = 1 if (neg_div_after_first and j > 0) else 0
                region = 0 if e.region == F32 else 1
                rows[j, 0], rows[j, 1], rows[j, 2] = flat, e.offset, e.numel
                rows[j, 3] = np.uint64(region | (flags << 32))
                flat += e.numel
            hit = (torch.from_numpy(rows.view(np.int64).copy()).to(eng.device), flat)
            lay._cache[key] = hit
        return hit

    def _flatten(self, mode: int, segs, n_segs: int, n_flat: int, src_f: Sequence[int], src_i: Sequence[int],
                 base: DeviceArena | None, lr: float, stream) -> torch.Tensor:
        """K flat vectors (rows of a [K, ``_flat_stride``] buffer) from device arenas, minus ``base``.
        ``None`` subtracts nothing: RAW, and DELTA over rows that already hold x - b (delta arenas).
        ``plato_agg_flatten`` takes both regions of a baseline or neither, whatever the layout holds."""
        eng = self.engine
        k = len(src_f)
        stride = _flat_stride(n_flat)
        out = torch.empty((k, stride), dtype=torch.float32, device=eng.device)
        ptrs = torch.from_numpy(np.asarray(list(src_f) + list(src_i) +
                                           [out.data_ptr() + r * stride * 4 for r in range(k)],
                                           dtype=np.int64)).to(eng.device)
        base_f, base_i = (None, None) if base is None else (base.f32.data_ptr(), base.i64.data_ptr())
        _lib.call("plato_agg_flatten", mode, ptrs.data_ptr(), ptrs.data_ptr() + 8 * k, k, base_f, base_i,
                  segs.data_ptr(), n_segs, n_flat, float(lr), ptrs.data_ptr() + 16 * k, stream.cuda_stream)
        self._keep_flat = ptrs
        return out

    def _fedadp_order(self):
        lay = self.layout
        order = fedadp_order(lay.keys())
        if order and lay.entries[order[0]].region != F32:
            raise ValueError("FedAdp: the first entry in name order is int64, so the reference flattens to "
                             "float64 (np.append) and takes float64 dots; the device path reproduces the "
                             "float32 case only")
        return order

    def fedadp_dots(self, grads: tuple[torch.Tensor, torch.Tensor], slots: Sequence[int], lr: float):
        """FedAdp's float32 reductions of process_grad's flattened vectors, bit-exact.

        ``grads`` is the device global gradient (fp32 arena, fp32 values of the
        int64 entries), e.g. :meth:`launch_entrywise` with ``device=True``.
        Returns ``(inner[K], g_sq, l_sq[K])`` as numpy float32: ``np.inner(g,
        loc_k)``, ``g.dot(g)``, ``loc_k.dot(loc_k)`` exactly as numpy's OpenBLAS
        forms them (examples/server_aggregation/fedadp/fedadp_server.py:91-99).
        The global gradient is flattened once (``plato_agg_flatten``, RAW); the
        clients' loc_k are gathered from their staged arenas inside
        ``plato_agg_fedadp_dots``, which runs the sdot chains with no flattened
        copies of the K deltas.
        """
        slots, _, _, stream = self._staged_rows(slots, tables=False)
        eng, lay = self.engine, self.layout
        order = self._fedadp_order()
        segs, n_flat = self._flat_segments(order, True)
        # plato_agg_fedadp_dots' limits (csrc/fedadp.hip run_fedadp); beyond them the round-2 path
        if (len(order) >= self.FEDADP_MAX_SEGS or n_flat >= 1 << 30 or lay.n_f32 >= 1 << 30
                or lay.n_i64 >= 1 << 30 or len(slots) > 65535
                or self.fedadp_boundary_rows(len(order), lay.n_i64) >= self.FEDADP_MAX_BND):
            return self.fedadp_dots_flat(grads, slots, lr)
        g_flat = self._flatten(_lib.PLATO_AGG_FLAT_RAW, segs, len(order), n_flat, [grads[0].data_ptr()],
                               [grads[1].data_ptr()], None, lr, stream)
        k = len(slots)
        ptrs = torch.from_numpy(np.asarray([self._pf[i] for i in slots] + [self._pi[i] for i in slots],
                                           dtype=np.int64)).to(eng.device)
        xy = torch.empty(k + 1, dtype=torch.float32, device=eng.device)
        yy = torch.empty(k + 1, dtype=torch.float32, device=eng.device)
        # The workspace's layout-only tables (descriptors, boundary rows and their sources) depend on the
        # segment map alone (`segs`, cached on the layout): the engine keeps its last workspace, and its next
        # round of the same layout and K skips building them (PLATO_AGG_FEDADP_TABLES_READY).  Per engine,
        # not per layout: an engine runs one round at a time, while several engines (a client-split round's
        # devices, repeated devices in tests) may reduce the same layout concurrently.
        ws_key = (id(lay), lay.signature, tuple(order), k, segs.data_ptr())
        held = getattr(eng, "_fedadp_ws", None)
        if held is not None and held[0] == ws_key and held[1] is lay:
            ws, flags = held[2], _lib.PLATO_AGG_FEDADP_TABLES_READY
        else:
            eng._fedadp_ws = None  # one workspace per engine (K varies between async rounds)
            ws = torch.empty(-(-_lib.lib().plato_agg_fedadp_dots_workspace(k, 1, lay.n_i64, n_flat, len(order)) // 4),
                             dtype=torch.float32, device=eng.device)
            flags = 0
        with self._timed("fedadp_dots", stream):
            # delta arenas: a null baseline selects the kernel that streams none (same values, same order)
            _lib.call("plato_agg_fedadp_dots_ex", g_flat.data_ptr(), ptrs.data_ptr(), ptrs.data_ptr() + 8 * k, k,
                      *self._baseline(self.deltas), segs.data_ptr(), len(order), n_flat,
                      lay.n_f32, lay.n_i64, float(lr), 1, ws.data_ptr(), xy.data_ptr(), yy.data_ptr(),
                      stream.cuda_stream, flags)
        xy_h, yy_h = xy.cpu().numpy(), yy.cpu().numpy()  # stream-ordered D2H (syncs this stream)
        eng._fedadp_ws = (ws_key, lay, ws)  # its tables are built (this stream has passed the call)
        self._resolve_timers()
        self._keep_flat = (g_flat, ptrs, ws)
        return xy_h[:k], xy_h[k], yy_h[:k]

    def fedadp_dots_flat(self, grads: tuple[torch.Tensor, torch.Tensor], slots: Sequence[int], lr: float,
                         batch_bytes: float = 32e9):
        """The same dots through materialised flat vectors (``plato_agg_flatten`` + ``plato_agg_sdot_shared``).

        The round-2 path, kept as an independent device cross-check of
        :meth:`fedadp_dots` (tests), for the before/after timing
        (scripts/bench_variant_paths.py), and for models beyond the fused
        kernel's limits (:meth:`fedadp_dots` falls back here).  On delta arenas
        the rows are flattened as they are (no baseline): they hold the fp32
        deltas and the exact int64 differences already.
        """
        slots, _, _, stream = self._staged_rows(slots, tables=False)
        eng = self.engine
        order = self._fedadp_order()
        segs, n_flat = self._flat_segments(order, True)
        g_flat = self._flatten(_lib.PLATO_AGG_FLAT_RAW, segs, len(order), n_flat, [grads[0].data_ptr()],
                               [grads[1].data_ptr()], None, lr, stream)
        stride = _flat_stride(n_flat)
        k = len(slots)
        # rows 0..k-1: g.loc_k and loc_k.loc_k; row k: g.g (the global gradient's squared norm),
        # which the last batch's launch forms alongside (with_xx)
        xy = torch.empty(k + 1, dtype=torch.float32, device=eng.device)
        yy = torch.empty(k + 1, dtype=torch.float32, device=eng.device)
        per = max(1, int(batch_bytes // (stride * 4)))
        ws = torch.empty(_lib.lib().plato_agg_sdot_shared_workspace(min(k, per), 1) // 4, dtype=torch.float32,
                         device=eng.device)
        keep = []
        for s0 in range(0, k, per):
            part = slots[s0:s0 + per]
            locs = self._flatten(_lib.PLATO_AGG_FLAT_DELTA, segs, len(order), n_flat, [self._pf[i] for i in part],
                                 [self._pi[i] for i in part], None if self.deltas else self._base, lr, stream)
            last = s0 + per >= k
            ys_h = [locs.data_ptr() + r * stride * 4 for r in range(len(part))]
            ys = torch.from_numpy(np.asarray(ys_h, dtype=np.int64)).to(eng.device)
            _lib.call("plato_agg_sdot_shared", g_flat.data_ptr(), ys.data_ptr(), len(ys_h), n_flat, int(last),
                      ws.data_ptr(), xy.data_ptr() + 4 * s0, yy.data_ptr() + 4 * s0, stream.cuda_stream)
            keep.append((locs, ys))
            if s0 + per < k:
                stream.synchronize()  # bound the flat buffers to one batch
                keep = []
        stream.synchronize()
        xy_h, yy_h = xy.cpu().numpy(), yy.cpu().numpy()
        inner, g_sq, l_sq = xy_h[:k], xy_h[k], yy_h[:k]
        return inner, g_sq, l_sq

    def np_sumsq(self, slots: Sequence[int]) -> np.ndarray:
        """numpy's float32 ``np.sum(np.square(x - b))`` of every fp32 entry, per client, bit-exact.

        Polaris' per-layer squared deltas (examples/client_selection/polaris/
        polaris_server.py:78-81) in numpy's own order (``plato_agg_np_sumsq``).
        Returns ``[K, E]`` float32 (entries in layout order; int64 entries 0).
        """
        slots, _, _, stream = self._staged_rows(slots, tables=False)
        eng, lay = self.engine, self.layout
        key = ("np_sumsq_pieces", str(eng.device))
        hit = lay._cache.get(key)
        if hit is None:
            rows, first, n_chunks = [], [], 0
            for idx, e in enumerate(lay.entries):
                if e.region == F32 and e.numel:
                    rows.append((idx, e.offset, e.offset + e.numel, 0))
                    first.append(n_chunks)
                    n_chunks += -(-e.numel // 8192)
            pieces = np.asarray(rows, dtype=np.uint32).reshape(-1, 4)
            hit = (torch.from_numpy(pieces.view(np.int32).copy()).to(eng.device),
                   torch.from_numpy(np.asarray(first, dtype=np.uint32).view(np.int32)).to(eng.device),
                   pieces[:, 0].astype(np.int64), n_chunks)
            lay._cache[key] = hit
        pieces, first, entry_of, n_chunks = hit
        k, n_p = len(slots), int(entry_of.size)
        out = np.zeros((k, len(lay.entries)), dtype=np.float32)
        if n_p == 0:
            return out
        tf = torch.from_numpy(np.asarray([self._pf[i] for i in slots], dtype=np.int64)).to(eng.device)
        ws = torch.empty(max(1, eng.lib.plato_agg_np_sumsq_workspace(k, n_chunks) // 4), dtype=torch.float32,
                         device=eng.device)
        dev_out = torch.empty((k, n_p), dtype=torch.float32, device=eng.device)
        with self._timed("np_sumsq", stream):
            # delta arenas: a null baseline selects the kernels that load none (the rows hold x - b)
            _lib.call("plato_agg_np_sumsq", tf.data_ptr(), k, self._baseline(self.deltas)[0], pieces.data_ptr(),
                      first.data_ptr(), n_p, n_chunks, ws.data_ptr(), dev_out.data_ptr(), stream.cuda_stream)
        out[:, entry_of] = dev_out.cpu().numpy()
        self._resolve_timers()
        return out

    PORT_NORMS_MAX_SEGS = 2048  # csrc/port.hip kMaxSegs
    FEDADP_MAX_SEGS = 1 << 22   # csrc/fedadp.hip run_fedadp
    FEDADP_MAX_BND = 1 << 22    # boundary-table rows (32-bit byte offsets of 1 KiB rows)

    @staticmethod
    def fedadp_boundary_rows(n_segs: int, n_i64: int) -> int:
        """csrc/fedadp.hip adp_max_bnd: boundary-table rows the kernel reserves per pair."""
        return 2 * (n_segs + n_i64 // 256 + 1)

    def model_similarities(self, reference: Mapping[str, torch.Tensor], slots: Sequence[int],
                           eps: float = 1e-8, threads: int | None = None, flat_norms: bool = False) -> list[np.float32]:
        """Port's cosine similarity of each client delta with ``baseline - reference``, bit-exact.

        ``F.cosine_similarity(current - previous, delta, dim=0)`` over the
        models flattened by ``torch.cat`` in state_dict order
        (examples/async/port/port_server.py:24-52), computed on the device in
        the order x86-64 PyTorch 2.10 uses on ``threads`` CPU threads (default
        ``torch.get_num_threads()``: what the reference's call would use in this
        process).  ``plato_agg_port_norms`` gathers ``current - previous`` and
        every client delta straight from the staged arenas for the vector norms
        (serial-chain bound) and stores the flattened vectors as it goes; the
        cascade cosine sums (``plato_agg_torch_cosine_sum``) then read those.
        ``flat_norms=True`` runs the round-2 path instead — ``plato_agg_flatten``,
        then ``plato_agg_entry_norms_f32`` over the flat rows — kept as a device
        cross-check.
        Returned as fp32 like the reference's 0-dim tensor.
        """
        if not self.has_baseline:
            raise ValueError("baseline not staged")
        slots = list(slots)
        if not slots:
            return []
        slots, _, _, stream = self._staged_rows(slots, tables=False)
        threads = torch.get_num_threads() if threads is None else int(threads)
        eng = self.engine
        lay = self.layout
        if isinstance(reference, DeviceArena):  # staged ahead by stage_reference
            if reference.layout is not lay:
                raise ValueError("reference arena was staged for another round / layout")
            prev = reference
        else:
            prev = self._stage_model(reference, "reference model", stream)
        segs, n_flat = self._flat_segments(list(range(len(lay.entries))), False)
        n_segs = len(lay.entries)
        stride = _flat_stride(n_flat)
        k = len(slots)
        h = stream.cuda_stream
        # plato_agg_port_norms keeps the segment map in LDS (<= PORT_NORMS_MAX_SEGS entries) and takes
        # n_flat < 2^31, n_f32 < 2^30: larger models take the flatten + entry_norms path (same bits)
        if n_segs > self.PORT_NORMS_MAX_SEGS or n_flat >= 1 << 31 or lay.n_f32 >= 1 << 30:
            flat_norms = True
        norms = torch.empty(k + 1, dtype=torch.float32, device=eng.device)
        ws = torch.empty(max(1, eng.lib.plato_agg_torch_cosine_workspace(k, threads) // 4), dtype=torch.float32,
                         device=eng.device)
        out = torch.empty(k, dtype=torch.float32, device=eng.device)
        cur_f, cur_i = self._base.f32.data_ptr(), self._base.i64.data_ptr()  # the current model, as a vector
        if flat_norms:  # the round-2 path: flattened vectors, norms and sums over them
            cur = self._flatten(_lib.PLATO_AGG_FLAT_CAST_DIFF, segs, n_segs, n_flat, [cur_f], [cur_i], prev, 0.0,
                                stream)
            # (delta arenas: the rows as they are, int64 differences cast once as before)
            deltas = self._flatten(_lib.PLATO_AGG_FLAT_DELTA, segs, n_segs, n_flat, [self._pf[i] for i in slots],
                                   [self._pi[i] for i in slots], None if self.deltas else self._base, 0.0, stream)
            rows = [cur.data_ptr()] + [deltas.data_ptr() + r * stride * 4 for r in range(k)]
            tab = torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(eng.device)
            chunk = torch.from_numpy(np.asarray([[0, 0, n_flat, 0]], dtype=np.uint32).view(np.int32)).to(eng.device)
            # the rows are `stride` long (the padding past n_flat is read, never summed): declaring that length keeps
            # the one n_flat-long piece off the kernel's partial-last-float4 fallback (a per-wave path ~1.5x slower)
            _lib.call("plato_agg_entry_norms_f32", tab.data_ptr(), None, k + 1, None, None, chunk.data_ptr(), 1, None,
                      0, 1, stride, 0, norms.data_ptr(), h)
            _lib.call("plato_agg_torch_cosine_sum", cur.data_ptr(), tab.data_ptr() + 8, k, n_flat, norms.data_ptr(),
                      norms.data_ptr() + 4, float(eps), threads, ws.data_ptr(), out.data_ptr(), h)
            keep = (cur, deltas, tab, chunk)
        else:  # norms straight from the arenas; the same kernel stores the flattened vectors for the sums
            flat = torch.empty((k + 1, stride), dtype=torch.float32, device=eng.device)
            base_f, base_i = self._baseline(self.deltas)  # what the client vectors subtract: nothing on delta arenas
            vec = np.asarray([cur_f] + [self._pf[i] for i in slots]
                             + [cur_i] + [self._pi[i] or 0 for i in slots]
                             + [prev.f32.data_ptr()] + [base_f or 0] * k
                             + [prev.i64.data_ptr()] + [base_i or 0] * k
                             + [flat.data_ptr() + r * stride * 4 for r in range(k + 1)], dtype=np.int64)
            vt = torch.from_numpy(vec).to(eng.device)
            v8, n1 = vt.data_ptr(), 8 * (k + 1)
            scaled = torch.empty(stride, dtype=torch.float32, device=eng.device)
            args = (v8, v8 + n1, v8 + 2 * n1, v8 + 3 * n1, k + 1, None, segs.data_ptr(), n_segs, n_flat, lay.n_f32,
                    _lib.PLATO_AGG_PORT_CAST_FIRST, norms.data_ptr(), v8 + 4 * n1, h)
            with self._timed("port_norms", stream):
                if eng.port_variant is None:
                    _lib.call("plato_agg_port_norms", *args)
                else:
                    _lib.tune_call("plato_agg_tune_port_norms", eng.port_variant, *args)
            # current - previous over its norm once (not once per client), then the K cascade sums
            with self._timed("port_cosine", stream):
                _lib.call("plato_agg_scale_by_norm", flat.data_ptr(), n_flat, norms.data_ptr(), float(eps),
                          scaled.data_ptr(), h)
                _lib.call("plato_agg_torch_cosine_sum_scaled", scaled.data_ptr(), v8 + 4 * n1 + 8, k, n_flat,
                          norms.data_ptr() + 4, float(eps), threads, ws.data_ptr(), out.data_ptr(), h)
            keep = (vt, flat, scaled)
        stream.synchronize()
        self._resolve_timers()
        del keep
        self.last_norms = norms.cpu().numpy()
        return [np.float32(v) for v in out.cpu().numpy()]
