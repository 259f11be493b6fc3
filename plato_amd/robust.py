"""The detector example's robust aggregators (examples/detector/aggregations.py): Median, Trimmed-mean,
Multi-krum, Bulyan and Fl-trust.  All have one shape: K native payloads staged as weights (no baseline),
pointer tables of the rows, one to three kernels with at most one blocking read for a decision taken on the
host (``plato_amd.krum``, ``plato_amd.trust``), an all-float32 result.  :class:`RobustLaunches` is that shape
as a mixin of ``engine.AggregationRound``, :class:`RobustAggregates` the one-call forms of ``FedAvgEngine``.
"""

from __future__ import annotations

import time
from collections import OrderedDict
from typing import Mapping, Sequence

import numpy as np
import torch

from . import _lib
from .arena import payload_codec
from .arrivals import adopt_or_put


class RobustLaunches:
    """``launch_*`` of the robust aggregators (mixin of ``AggregationRound``)."""

    def _robust_rows(self, what: str, order: Sequence[int] | None, whole_model: bool = True, check=None):
        """(slots, fp32 pointer table, int64 pointer table, stream) of a robust launch, the stream
        ordered behind the staged copies.  Every refusal comes before any GPU work; ``whole_model``
        adds those of the launches that sum over the flattened model, ``check(K)`` the caller's own."""
        if self.codec != "native":
            raise ValueError(f"robust aggregation takes native payloads; this round holds {self.codec} codes")
        self._raw_only(what)
        order = [i for i in range(self.capacity) if self.staged[i]] if order is None else list(order)
        slots = self._check_slots(order)
        if whole_model:
            if len(slots) > _lib.PLATO_AGG_ROBUST_MAX_K:
                raise ValueError(f"robust aggregation takes at most {_lib.PLATO_AGG_ROBUST_MAX_K} clients, "
                                 f"got {len(slots)}")
            if not self.layout.packed:
                raise ValueError(f"{what} sums over the whole fp32 region: the arena must have no alignment padding")
        if check is not None:
            check(len(slots))
        tf, ti = self._row_tables(slots)
        stream = torch.cuda.current_stream(self.engine.device)
        self.stager.fence(stream)
        return slots, tf, ti, stream

    def _launch_rows(self, what: str, order, body, whole_model: bool = True, check=None) -> None:
        """The robust launches' common path: the rows of :meth:`_robust_rows`, then
        ``body(slots, tf, ti, stream)`` enqueues the kernels between the round's event pair and returns
        the two output rows and the device buffers to keep alive until the result is fetched."""
        slots, tf, ti, stream = self._robust_rows(what, order, whole_model, check)
        self.timings["stage_ms"] = (time.perf_counter() - self._t0) * 1e3
        self._k = len(slots)  # algorithmic_bytes: a body that reads the rows more than once says so
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        out_f, out_i, keep = body(slots, tf, ti, stream)
        e1.record(stream)
        self._kernel_events = (e0, e1)
        self._robust = True
        self._fetch(stream, out_f, out_i, (tf, ti, *keep))

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

    def _sizes(self, stream):  # the tail of a kernel call
        return self.layout.n_f32, self.layout.n_i64, stream.cuda_stream

    def _robust_columns(self, mode: str, tf, ti, k: int, trim: int, out_f, out_i, stream) -> None:
        with self._timed("robust_" + mode, stream):
            _lib.call("plato_agg_robust_columns", _lib.PLATO_AGG_ROBUST[mode], *self._regions(tf, ti), k, int(trim),
                      *self._regions(out_f, out_i), *self._sizes(stream))

    def _mean_rows(self, tf, ti, m: int, out_f, out_i, stream) -> None:
        with self._timed("mean_rows", stream):
            _lib.call("plato_agg_mean_rows", *self._regions(tf, ti), m, *self._regions(out_f, out_i),
                      *self._sizes(stream))

    def launch_robust(self, mode: str = "median", trim: int = 0, order: Sequence[int] | None = None) -> None:
        """Coordinate-wise robust aggregation of the staged client rows (``plato_agg_robust_columns``).

        ``mode="median"`` is ``aggregations.median`` of the reference's detector example
        (examples/detector/aggregations.py): ``torch.median(dim=0)`` of the flattened models, the
        lower median per coordinate.  ``mode="nearest_mean"`` is ``aggregations.trimmed_mean``: per
        coordinate the mean of the ``K - 2 * trim`` values nearest that median, equally distant ones
        taken in table order (``0 <= 2 * trim < K``; the reference's own ``num_attackers`` is 0).  No
        baseline is read.  Every entry of the result is float32, the int64 counters included
        (``flatten_weights`` promotes them).
        """
        if mode not in _lib.PLATO_AGG_ROBUST:
            raise ValueError(f"unknown robust aggregation mode {mode!r} (supported: {sorted(_lib.PLATO_AGG_ROBUST)})")

        def body(slots, tf, ti, stream):
            out_f, out_i = self._out_rows()
            self._robust_columns(mode, tf, ti, len(slots), trim, out_f, out_i, stream)
            return out_f, out_i, ()

        # per coordinate: a padded layout will do, and the C side refuses a K it cannot take
        self._launch_rows("launch_robust", order, body, whole_model=False)

    def _pairwise_sqdist(self, k: int, tf, ti, stream) -> np.ndarray:
        lay, dev = self.layout, self.engine.device
        nbytes = _lib.lib().plato_agg_pairwise_sqdist_workspace(k, lay.n_f32, lay.n_i64)
        work = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
        out = torch.empty((k, k), dtype=torch.float64, device=dev)
        with self._timed("pairwise_sqdist", stream):
            _lib.call("plato_agg_pairwise_sqdist", *self._regions(tf, ti), k, lay.n_f32, lay.n_i64,
                      work.data_ptr(), out.data_ptr(), stream.cuda_stream)
        dist = out.cpu().numpy()  # stream-ordered, blocking: the selection runs on the host
        del work
        return dist

    def launch_pairwise_sqdist(self, order: Sequence[int] | None = None) -> np.ndarray:
        """The [K, K] float64 matrix of squared L2 distances between the staged client rows, over the
        whole flattened model (``plato_agg_pairwise_sqdist``): entry [i, j] is
        ``torch.norm(x_order[i] - x_order[j]) ** 2`` of the reference's distance-based aggregators and
        detectors (examples/detector/aggregations.py:185-192), with fp32 differences and a float64
        sum.  Synchronises: the matrix is returned on the host."""
        slots, tf, ti, stream = self._robust_rows("launch_pairwise_sqdist", order)
        dist = self._pairwise_sqdist(len(slots), tf, ti, stream)
        self._resolve_timers()
        return dist

    def _launch_selected(self, what: str, order, check, select, combine) -> None:
        """The distance-based aggregators: ``check(K)`` refuses a K too small, the distance matrix is
        computed on the device, ``select(dist)`` picks rows on the host, and
        ``combine(sf, si, m, out_f, out_i, stream)`` launches the kernel that turns the pointer tables of
        the m selected rows, in selection order, into the result."""

        def body(slots, tf, ti, stream):
            dist = self._pairwise_sqdist(len(slots), tf, ti, stream)
            t0 = time.perf_counter()
            picks = select(dist)
            self.timings["select_ms"] = (time.perf_counter() - t0) * 1e3
            self.selected = self.engine.last_selected = [slots[p] for p in picks]
            self._k = len(slots) + len(picks)  # K rows for the distances, then the selected ones again
            sf, si = self._row_tables(self.selected)
            out_f, out_i = self._out_rows()
            combine(sf, si, len(picks), out_f, out_i, stream)
            return out_f, out_i, (sf, si)

        self._launch_rows(what, order, body, check=check)

    def launch_multi_krum(self, f: int = 2, order: Sequence[int] | None = None) -> None:
        """``aggregations.multi_krum`` of the reference's detector example over the staged client rows:
        the distance matrix on the device, the selection on the host (``plato_amd.krum``), then the mean
        of the selected rows in selection order (``plato_agg_mean_rows``).  ``self.selected`` holds the
        selected client slots in selection order.  No baseline is read; every entry of the result is
        float32, the int64 counters included."""
        from .krum import multi_krum_select

        f = int(f)

        def check(k):
            if k <= 2 * f + 2:
                raise ValueError(f"Multi-Krum with f = {f} needs more than {2 * f + 2} clients, got {k}")

        self._launch_selected("launch_multi_krum", order, check, lambda dist: multi_krum_select(dist, f),
                              self._mean_rows)

    def launch_bulyan(self, f: int, order: Sequence[int] | None = None) -> None:
        """``aggregations.bulyan`` of the reference's detector example over the staged client rows: the
        distance matrix on the device, the selection of theta = min(K - 2f, K - 2 - f) clients on the
        host (``plato_amd.krum.bulyan_select``), then per coordinate the mean of the theta - 2f selected
        values nearest their median (``plato_agg_robust_columns``, nearest-mean mode, over the selected
        rows in selection order).  ``self.selected`` holds the selected client slots in selection order.
        No baseline is read; every entry of the result is float32, the int64 counters included."""
        from .krum import bulyan_min_clients, bulyan_select

        f = int(f)

        def check(k):
            if f < 0 or k < bulyan_min_clients(f):
                raise ValueError(f"Bulyan with f = {f} needs at least {bulyan_min_clients(max(f, 0))} clients, got {k}")

        self._launch_selected("launch_bulyan", order, check, lambda dist: bulyan_select(dist, f),
                              lambda sf, si, m, *out: self._robust_columns("nearest_mean", sf, si, m, f, *out))

    def launch_fltrust(self, order: Sequence[int] | None = None) -> None:
        """``aggregations.fl_trust`` of the reference's detector example over the staged client rows: the
        sequential mean of the rows (``plato_agg_mean_rows``), every client's dot with it and the norms
        in one pass (``plato_agg_trust_stats``), the cosines, their clip and normalisation on the host
        (``plato_amd.trust.fltrust_weights``, after a blocking read of the ``3K + 1`` sums), then the sum
        of the rows scaled by ``w_k / |x_k + 1e-9| * |mean|`` in table order (``plato_agg_scaled_sum``).
        ``self.trust`` holds the scalars.  No baseline is read; every entry of the result is float32,
        the int64 counters included."""
        from .trust import EPS, fltrust_weights

        def body(slots, tf, ti, stream):
            lay, dev, k = self.layout, self.engine.device, len(slots)
            self._k = 3 * k  # the rows are read by the mean, the statistics and the sum
            mean_f, mean_i = self._out_rows()
            self._mean_rows(tf, ti, k, mean_f, mean_i, stream)
            nbytes = _lib.lib().plato_agg_trust_stats_workspace(k, lay.n_f32, lay.n_i64)
            work = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
            stats = torch.empty(3 * k + 1, dtype=torch.float64, device=dev)
            with self._timed("trust_stats", stream):
                _lib.call("plato_agg_trust_stats", *self._regions(tf, ti), k, *self._regions(mean_f, mean_i), EPS,
                          lay.n_f32, lay.n_i64, work.data_ptr(), stats.data_ptr(), stream.cuda_stream)
            host_stats = stats.cpu().numpy()  # stream-ordered, blocking: the scalars are formed on the host
            t0 = time.perf_counter()
            self.trust = self.engine.last_trust = fltrust_weights(host_stats, k, EPS)
            self.timings["trust_scalars_ms"] = (time.perf_counter() - t0) * 1e3
            scal = torch.from_numpy(np.concatenate([self.trust["weights"], self.trust["div"]])).to(dev)
            out_f, out_i = self._out_rows()
            with self._timed("trust_combine", stream):
                _lib.call("plato_agg_scaled_sum", *self._regions(tf, ti), k, scal.data_ptr(), scal.data_ptr() + 4 * k,
                          float(self.trust["nm"]), *self._regions(out_f, out_i), *self._sizes(stream))
            return out_f, out_i, (mean_f, mean_i, work, stats, scal)

        self._launch_rows("launch_fltrust", order, body)


class RobustAggregates:
    """``aggregate_*`` of the robust aggregators over CPU payloads (mixin of ``FedAvgEngine``)."""

    def _stage_selected(self, payloads: Sequence[Mapping[str, torch.Tensor]]):
        """A round with K native payloads staged as weights, for the robust aggregators."""
        k = len(payloads)
        if k == 0:
            raise ValueError("no client payloads to aggregate")
        if k > _lib.PLATO_AGG_ROBUST_MAX_K:
            raise ValueError(f"robust aggregation takes at most {_lib.PLATO_AGG_ROBUST_MAX_K} clients, got {k}")
        codec = payload_codec(payloads[0])
        if codec != "native":
            raise ValueError(f"robust aggregation takes native payloads, not {codec} codes")
        rnd = self.begin(payloads[0], k)
        rnd.deltas = False  # no baseline: the rows stay weights
        adopt_or_put(rnd, payloads)
        return rnd

    def aggregate_robust(self, payloads: Sequence[Mapping[str, torch.Tensor]], mode: str = "median",
                         trim: int = 0) -> "OrderedDict[str, torch.Tensor]":
        """The detector example's order-statistic aggregators over K native payloads, on the GPU.

        ``mode="median"``: the coordinate-wise lower median (``aggregations.median``).
        ``mode="nearest_mean"``: the mean of the ``K - 2 * trim`` values nearest that median
        (``aggregations.trimmed_mean``, whose own ``num_attackers`` is 0).  Returns CPU float32 tensors
        for every entry, the int64 counters included, as the reference does.
        """
        rnd = self._stage_selected(payloads)
        rnd.launch_robust(mode, trim)
        return rnd.result()

    def aggregate_multi_krum(self, payloads: Sequence[Mapping[str, torch.Tensor]], f: int = 2
                             ) -> "OrderedDict[str, torch.Tensor]":
        """The detector example's ``Multi-krum`` (``aggregations.multi_krum``) over K native payloads, on
        the GPU: the mean of the ``K - 2f - 2`` clients its distance scores select.  Returns CPU float32
        tensors for every entry, the int64 counters included, as the reference does."""
        if 0 < len(payloads) <= 2 * int(f) + 2:
            raise ValueError(f"Multi-Krum with f = {int(f)} needs more than {2 * int(f) + 2} clients, "
                             f"got {len(payloads)}")
        rnd = self._stage_selected(payloads)
        rnd.launch_multi_krum(f)  # sets self.last_selected
        return rnd.result()

    def aggregate_bulyan(self, payloads: Sequence[Mapping[str, torch.Tensor]], f: int
                         ) -> "OrderedDict[str, torch.Tensor]":
        """The detector example's ``Bulyan`` (``aggregations.bulyan``) over K native payloads, on the GPU:
        its distance scores select theta = min(K - 2f, K - 2 - f) clients, and every coordinate is the
        mean of the theta - 2f selected values nearest their median.  K, the reference's
        ``clients.total_clients``, is the number of payloads.  Returns CPU float32 tensors for every
        entry, the int64 counters included, as the reference does."""
        from .krum import bulyan_min_clients

        if payloads and (int(f) < 0 or len(payloads) < bulyan_min_clients(f)):
            raise ValueError(f"Bulyan with f = {int(f)} needs at least {bulyan_min_clients(max(int(f), 0))} clients, "
                             f"got {len(payloads)}")
        rnd = self._stage_selected(payloads)
        rnd.launch_bulyan(f)  # sets self.last_selected
        return rnd.result()

    def aggregate_fltrust(self, payloads: Sequence[Mapping[str, torch.Tensor]]
                          ) -> "OrderedDict[str, torch.Tensor]":
        """The detector example's ``Fl-trust`` (``aggregations.fl_trust``) over K native payloads, on the
        GPU: every client weighed by its clipped cosine with the mean model and rescaled to the mean's
        norm.  ``self.last_trust`` holds the scalars (``plato_amd.trust.fltrust_weights``).  Returns CPU
        float32 tensors for every entry, the int64 counters included, as the reference does."""
        rnd = self._stage_selected(payloads)
        rnd.launch_fltrust()
        return rnd.result()
