"""The detector example's robust aggregators (examples/detector/aggregations.py): Median, Trimmed-mean,
Multi-krum, Bulyan and Fl-trust.  All have one shape: K native payloads staged as weights (no baseline),
pointer tables of the rows, one to three kernels with at most one blocking read for a decision taken on the
host (``plato_amd.krum``, ``plato_amd.trust``), an all-float32 result.  :class:`RobustLaunches` is that shape
as a mixin of ``engine.AggregationRound``, :class:`RobustAggregates` the one-call forms of ``FedAvgEngine``.
``launch_attack`` is the attack simulation that the example runs before them (examples/detector/attacks.py):
it poisons the attackers' staged rows in place, and the aggregators then read those rows.
``launch_fldetector`` is the defence that runs between the two (examples/detector/detectors.py: fl_detector):
it scores the staged rows against the engine's record (``plato_amd.detectors``) and changes none.
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
        """``_staged_rows`` of a robust launch (weights, no baseline; default: every staged slot) with
        the robust refusals, all before any kernel; ``whole_model`` adds those of the launches that sum
        over the flattened model, ``check(K)`` the caller's own."""
        if self.codec != "native":
            raise ValueError(f"robust aggregation takes native payloads; this round holds {self.codec} codes")
        self._raw_only(what)
        order = [i for i in range(self.capacity) if self.staged[i]] if order is None else order
        slots, tf, ti, stream = self._staged_rows(order, baseline=False)
        if whole_model:
            if len(slots) > _lib.PLATO_AGG_ROBUST_MAX_K:
                raise ValueError(f"robust aggregation takes at most {_lib.PLATO_AGG_ROBUST_MAX_K} clients, "
                                 f"got {len(slots)}")
            if not self.layout.packed:
                raise ValueError(f"{what} sums over the whole fp32 region: the arena must have no alignment padding")
        if check is not None:
            check(len(slots))
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
            with self._timed("trust_stats", stream):
                stats, work = self._trust_stats(tf, ti, k, mean_f, mean_i, lay.n_f32, lay.n_i64, stream, EPS)
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

    def _trust_stats(self, tf, ti, k: int, ref_f, ref_i, n_f32: int, n_i64: int, stream, eps: float = 0.0):
        """([3k + 1] float64 on the device, the workspace to keep until they are read):
        ``plato_agg_trust_stats`` of k rows against a vector."""
        dev = self.engine.device
        nbytes = _lib.lib().plato_agg_trust_stats_workspace(k, n_f32, n_i64)
        work = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
        stats = torch.zeros(3 * k + 1, dtype=torch.float64, device=dev)  # nothing is written for no coordinates
        _lib.call("plato_agg_trust_stats", tf.data_ptr() if n_f32 else None, ti.data_ptr() if n_i64 else None, k,
                  ref_f.data_ptr() if n_f32 else None, ref_i.data_ptr() if n_i64 else None, eps, n_f32, n_i64,
                  work.data_ptr(), stats.data_ptr(), stream.cuda_stream)
        return stats, work

    def launch_attack(self, kind: str, attackers: Sequence[int], *, per_round: int | None = None,
                      lambada_value: float | None = None) -> None:
        """The attack simulation of the reference's detector example (examples/detector/attacks.py) over
        the staged rows of the attackers, given as slots in ``self.updates`` order: their weight rows are
        poisoned in place, every other row stays as it is.

        ``kind`` is ``"lie"`` (``per_round`` = ``clients.per_round``), ``"lambda"`` (``lambada_value`` =
        ``clients.lambada_value``), ``"minmax"`` or ``"minsum"`` (``plato_amd.attacks.KINDS``).  The round
        holds weights and its baseline: the attackers' deltas x - b are formed in scratch rows
        (``plato_agg_compute_deltas``), the vector of the attack over them (``plato_agg_column_std``,
        ``plato_agg_mean_rows``; the unit vector of Min-Max and Min-Sum by ``plato_agg_scale_by_norm``, their
        lambda on the host from ``plato_agg_pairwise_sqdist`` and ``plato_agg_trust_stats``), and
        ``plato_agg_add_scaled_rows`` adds it to the weight rows.  LIE with one attacker changes nothing, as
        in the reference.  ``self.attack`` holds the scalars and the vector's two device regions
        (``"vector"``).  Runs on the round's one device; the launches that follow (``launch_robust`` and the
        others) read the poisoned rows."""
        from . import attacks

        if kind not in attacks.KINDS.values():
            raise ValueError(f"unknown attack {kind!r} (supported: {sorted(attacks.KINDS.values())})")
        if kind == "lie" and per_round is None:
            raise ValueError("the LIE attack needs per_round (clients.per_round)")
        if kind == "lambda" and lambada_value is None:
            raise ValueError("the Lambda attack needs lambada_value (clients.lambada_value)")
        if not self.has_baseline:
            raise ValueError("launch_attack forms the attackers' deltas: stage the baseline first")
        slots, tf, ti, stream = self._robust_rows("launch_attack", attackers)
        lay, dev, a = self.layout, self.engine.device, len(slots)
        self.attack = self.engine.last_attack = {"kind": kind, "attackers": slots, "poisoned": False}
        if kind == "lie" and a == 1:  # "LIE attack does not apply to solo attacker"
            return
        n_f, n_i, h = lay.n_f32, lay.n_i64, stream.cuda_stream
        base = self._base
        df = torch.empty((a, lay.row_f32), dtype=torch.float32, device=dev)
        di = torch.empty((a, lay.row_i64), dtype=torch.int64, device=dev)
        with self._timed("attack_deltas", stream):
            for j, slot in enumerate(slots):
                _lib.call("plato_agg_compute_deltas", self._pf[slot], self._pi[slot] if n_i else None,
                          base.f32.data_ptr(), base.i64.data_ptr() if n_i else None, df[j].data_ptr(),
                          di[j].data_ptr() if n_i else None, n_f, n_i, h)
        dtf, dti = self.engine._pointer_tables(
            np.asarray([df[j].data_ptr() for j in range(a)], dtype=np.int64),
            np.asarray([di[j].data_ptr() for j in range(a)], dtype=np.int64))
        v_f, v_i = self._out_rows()
        info = self.attack
        if kind == "lie":
            with self._timed("column_std", stream):
                _lib.call("plato_agg_column_std", *self._regions(dtf, dti), a, *self._regions(v_f, v_i),
                          *self._sizes(stream))
            info["z"] = attacks.lie_z(per_round, a)
            s = -np.float32(info["z"])
        elif kind == "lambda":
            self._mean_rows(dtf, dti, a, v_f, v_i, stream)
            s = -np.float32(lambada_value)
        else:
            minsum = kind == "minsum"
            avg_f, avg_i = self._out_rows()
            self._mean_rows(*((tf, ti) if minsum else (dtf, dti)), a, avg_f, avg_i, stream)  # Min-Sum: of the weights
            with self._timed("attack_stats", stream):
                s_avg, w0 = self._trust_stats(dtf, dti, a, avg_f, avg_i, n_f, n_i, stream)
            h_avg = s_avg.cpu().numpy()  # stream-ordered, blocking: the norm is rounded on the host
            with np.errstate(invalid="ignore"):
                norm = np.float32(np.sqrt(h_avg[3 * a]))  # float64 root, rounded to fp32 once
            d_norm = torch.from_numpy(np.asarray([norm], dtype=np.float32)).to(dev)
            with self._timed("attack_unit", stream):
                _lib.call("plato_agg_scale_by_norm", avg_f.data_ptr(), n_f, d_norm.data_ptr(), 0.0, v_f.data_ptr(), h)
                if n_i:
                    _lib.call("plato_agg_scale_by_norm", avg_i.data_ptr(), n_i, d_norm.data_ptr(), 0.0,
                              v_i.data_ptr(), h)
            # avg against p: avg's two regions are fp32, each a one-row table of an fp32 region
            atab = torch.tensor([avg_f.data_ptr(), avg_i.data_ptr()], dtype=torch.int64, device=dev)
            with self._timed("attack_stats_unit", stream):
                s_p, w1 = self._trust_stats(dtf, dti, a, v_f, v_i, n_f, n_i, stream)
                s_af, w2 = self._trust_stats(atab[:1], None, 1, v_f, None, n_f, 0, stream)
                s_ai, w3 = self._trust_stats(atab[1:], None, 1, v_i, None, n_i, 0, stream)
            dist = self._pairwise_sqdist(a, dtf, dti, stream)  # blocking: the statistics above are done too
            h_p, h_af, h_ai = s_p.cpu().numpy(), s_af.cpu().numpy(), s_ai.cpu().numpy()
            t0 = time.perf_counter()
            stats = attacks.SearchStats(uu=h_avg[a:2 * a], ua=h_avg[:a], up=h_p[:a], aa=float(h_avg[3 * a]),
                                        pp=float(h_p[3 * a]), ap=float(h_af[0] + h_ai[0]))
            lam = (attacks.min_sum_lambda if minsum else attacks.min_max_lambda)(stats, dist)
            self.timings["attack_search_ms"] = (time.perf_counter() - t0) * 1e3
            info.update(lam=lam, norm=norm, stats=stats,
                        threshold=(attacks.min_sum_threshold if minsum else attacks.min_max_threshold)(dist))
            # -1 * lambda_succ with the reference's integer 0 when nothing succeeded: +0, not -0
            s = lam if minsum else (np.float32(0.0) if lam == 0 else -lam)
            del w0, w1, w2, w3, atab
        with self._timed("add_scaled_rows", stream):
            _lib.call("plato_agg_add_scaled_rows", *self._regions(tf, ti), a, float(s), *self._regions(v_f, v_i),
                      *self._sizes(stream))
        info.update(s=np.float32(s), vector=(v_f[:n_f], v_i[:n_i]), poisoned=True)
        self._attack_keep = (df, di, dtf, dti, tf, ti)  # until the stream has passed the launches

    def launch_fldetector(self, received_ids: Sequence, order: Sequence[int] | None = None) -> None:
        """``detectors.fl_detector`` of the reference's detector example (examples/detector/detectors.py:
        310-418) over the staged client rows, ``received_ids`` their client ids in the same order.  The
        round holds weights and its baseline.  One pass forms the mean update, the mean step and the
        record's next rows (``plato_agg_detect_means``), one the dots that extend the record's Gram cache
        and give the right-hand side (``plato_agg_rows_dots``); the 2N x 2N system is solved on the host
        (``plato_amd.detectors``), ``plato_agg_lbfgs_predict`` forms the predicted update and
        ``plato_agg_delta_sqdist`` every client's squared distance to it; the scores and their 2-means
        split are the host's.  The record (``engine.fldetector``, a
        :class:`plato_amd.detectors.FLDetectorState`) is kept across rounds; the first round only starts
        it and flags nobody.  ``self.detector`` holds ``distances``, ``scores``, ``malicious`` (positions
        in ``order``), ``sigma``, ``cond`` and the device regions of the prediction (``pred``).
        Synchronises; nothing is aggregated and no row is changed."""
        from .detectors import FLDetectorState

        if not self.has_baseline:
            raise ValueError("launch_fldetector forms the clients' deltas: stage the baseline first")
        slots, tf, ti, stream = self._robust_rows("launch_fldetector", order)
        received_ids = list(received_ids)
        if len(received_ids) != len(slots):
            raise ValueError(f"launch_fldetector: {len(received_ids)} client ids for {len(slots)} rows")
        engine = self.engine
        if engine.fldetector is None:
            engine.fldetector = FLDetectorState()
        state = engine.fldetector
        try:
            self.detector = engine.last_detector = state.round(self, tf, ti, len(slots), received_ids, stream)
        finally:
            stream.synchronize()
            self._resolve_timers()

    def fetch_rows(self, slots: Sequence[int]):
        """[(fp32 region, int64 region)] of the staged rows ``slots`` as host tensors, stream-ordered
        behind the launches so far (the poisoned rows after :meth:`launch_attack`).  Blocks."""
        slots = self._check_slots(slots)
        stream = torch.cuda.current_stream(self.engine.device)
        self.stager.fence(stream)
        lay = self.layout
        out = []
        for slot in slots:
            row_f, row_i = self._row_tensors(slot)
            out.append((row_f[: lay.n_f32].cpu(), row_i[: lay.n_i64].cpu()))
        self._resolve_timers()
        return out

    def _row_tensors(self, slot: int):
        """The device tensors of a staged slot's rows: in the round's slab, or an arrival slab."""
        slab, row = self._rows[slot]
        return slab.f32[row], slab.i64[row]


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
