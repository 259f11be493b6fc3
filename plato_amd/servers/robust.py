"""Byzantine-robust aggregation hook: the order-statistic aggregators of the reference's detector example.

``examples/detector/detector_server.py`` dispatches ``aggregate_weights`` on
``server.secure_aggregation_type`` to ``examples/detector/aggregations.py``.  Its ``Median`` is a
coordinate-wise order statistic over the received models, not a weighted sum; here it runs on the GPU
(``plato_agg_robust_columns``).  Its ``Multi-krum`` scores every client by its squared distances to the
others and averages the selected ones: distances and mean on the GPU (``plato_agg_pairwise_sqdist``,
``plato_agg_mean_rows``), the selection on the host (``plato_amd.krum``).  Its ``Trimmed-mean`` and
``Bulyan`` end in the mean of the values nearest the coordinate-wise median (the nearest-mean mode of
``plato_agg_robust_columns``), ``Bulyan`` after a selection of Multi-krum's kind; they are
:class:`DetectorAggregationMixin`'s, which adds them to its parent's names.  Its ``Fl-trust`` weighs
every client by its clipped cosine with the mean model (``plato_agg_mean_rows``,
``plato_agg_trust_stats``, the scalars on the host in ``plato_amd.trust``, ``plato_agg_scaled_sum``); it is
:class:`TrustAggregationMixin`'s, which again adds it to its parent's.  One ``aggregate_weights`` serves
the three: a class differs in its table of names only.  The detector server's ``weights_received``
pipeline runs before this hook: its attack simulation (``weights_attacked``) runs on the GPU with
:class:`AttackSimulationMixin` for the attacks "LIE", "Lambda_attack", "Min-Max" and "Min-Sum"
(``plato_amd.attacks``), its filter (``weights_filter``) with :class:`DetectorFilterMixin` for the defence
"FLDetector" (``plato_amd.detectors``); every other attack and defence is the base class's, unchanged::

    Server = make_server(base=detector_server.Server, mixin=RobustAggregationMixin)

    class Mixin(DetectorFilterMixin, AttackSimulationMixin, DetectorAggregationMixin):
        pass
    Server = make_server(base=detector_server.Server, mixin=Mixin)
"""

from __future__ import annotations

from .. import tracing
from ..arena import payload_codec
from ..arrivals import adopt_or_put, stage_as_arrivals
from .fedavg import FusedAggregationMixin, _EngineHolder


def _secure_aggregation_type():
    try:
        from plato.config import Config

        server = Config().server
        return getattr(server, "secure_aggregation_type", None) if hasattr(server, "secure_aggregation_type") else None
    except Exception:  # Plato not importable / not configured: the FedAvg branch
        return None


def _num_attackers() -> int:
    """``len(Config().clients.attacker_ids)``, as ``aggregations.bulyan`` reads it (aggregations.py:80)."""
    from plato.config import Config

    return len(Config().clients.attacker_ids)


# An aggregator takes the server and returns the launch on the staged round.  It reads what it needs from
# the server before the engine is touched: a missing ``Config`` fails with nothing staged.
def _median(server):
    return lambda rnd: rnd.launch_robust("median")


def _multi_krum(server):
    return lambda rnd: rnd.launch_multi_krum(2)  # the reference's hard-coded num_attackers_selected (aggregations.py:180)


def _bulyan(server):
    f = int(server.num_attackers) if server.num_attackers is not None else _num_attackers()
    return lambda rnd: rnd.launch_bulyan(f)


def _trimmed_mean(server):
    return lambda rnd: rnd.launch_robust("nearest_mean", int(server.trim))


def _fl_trust(server):
    return lambda rnd: rnd.launch_fltrust()


class RobustAggregationMixin(FusedAggregationMixin):
    """``aggregate_weights`` hook of the detector server: "Median" and "Multi-krum" on the GPU, else the
    fused FedAvg."""

    #: None = ``Config().server.secure_aggregation_type`` (absent: FedAvg, as in the reference)
    secure_aggregation_type = None
    #: ``server.secure_aggregation_type`` -> aggregator; a subclass extends its parent's
    aggregators = {"Median": _median, "Multi-krum": _multi_krum}

    def robust_aggregation_type(self):
        own = self.secure_aggregation_type
        return own if own is not None else _secure_aggregation_type()

    async def aggregate_weights(self, updates, baseline_weights, weights_received):
        name = self.robust_aggregation_type()
        if name is None:  # the reference's "Fedavg is applied" branch
            return await super().aggregate_weights(updates, baseline_weights, weights_received)
        if name not in self.aggregators:
            raise ValueError(f"secure_aggregation_type {name!r} is not supported on the GPU "
                             f"(supported: {', '.join(sorted(self.aggregators))})")
        codec = payload_codec(weights_received[0])
        if codec != "native":
            raise ValueError(f"robust aggregation takes native payloads, not {codec} codes")
        engine = self.aggregation_engine()
        if getattr(engine, "primary", None) is not None:
            raise NotImplementedError("robust aggregation runs on one GPU (aggregation_devices has several)")
        launch = self.aggregators[name](self)
        try:
            rnd = engine.begin(weights_received[0], len(weights_received))

            def stage():
                with tracing.range("plato_amd.stage"):
                    adopt_or_put(rnd, weights_received)

            await self._off_loop(stage)
            with tracing.range("plato_amd.launch"):
                launch(rnd)
            with tracing.range("plato_amd.fetch"):
                return await self._finish(rnd)
        finally:
            engine.release_arrivals()


class DetectorAggregationMixin(RobustAggregationMixin):
    """``RobustAggregationMixin`` plus the detector example's "Bulyan" and "Trimmed-mean"; every other
    name is the parent's.

    "Bulyan" (aggregations.py:76-144): f is ``num_attackers`` if set, else
    ``len(Config().clients.attacker_ids)`` as in the reference.  K is the number of payloads received,
    where the reference reads ``clients.total_clients``: the two agree whenever every client reports,
    the only case in which the reference's loop is coherent (with fewer payloads than total_clients its
    cluster can outgrow the clients that remain).

    "Trimmed-mean" (aggregations.py:233-255): per coordinate the mean of the ``K - 2 * trim`` values
    nearest the median; ``trim`` defaults to 0, the reference's hard-coded ``num_attackers = 0``.
    """

    #: None = ``len(Config().clients.attacker_ids)``
    num_attackers = None
    trim = 0
    aggregators = {**RobustAggregationMixin.aggregators, "Bulyan": _bulyan, "Trimmed-mean": _trimmed_mean}


class TrustAggregationMixin(DetectorAggregationMixin):
    """``DetectorAggregationMixin`` plus the detector example's "Fl-trust" (aggregations.py:403-453);
    every other name is the parent's.  With it every working aggregator of that example runs on the GPU
    ("Krum" and "Afa" have no behaviour to match: INTEGRATION.md §12)."""

    aggregators = {**DetectorAggregationMixin.aggregators, "Fl-trust": _fl_trust}


def _clients_config(name: str):
    """``Config().clients.<name>``, or None where it is not set or Plato is not installed.  A
    configuration that fails to load raises: the round must not fall to the host path in silence."""
    try:
        from plato.config import Config
    except ImportError:
        return None
    return getattr(Config().clients, name, None)


class AttackSimulationMixin(_EngineHolder):
    """``weights_attacked`` of the detector server (detector_server.py:81-112) on the GPU, for the
    attacks ``attacks.get()`` can call with its four arguments and that draw nothing on the host: "LIE",
    "Lambda_attack", "Min-Max" and "Min-Sum".  Every other ``clients.attack_type`` ("Gassian_attack",
    "Fang", the "Oblivion-*" ones) and no attack at all go to the base class.

    The attackers' payloads are staged as arrival rows (or adopted, where they were staged at arrival),
    poisoned there in place (``AggregationRound.launch_attack``) and, by default, copied back into the
    payload tensors, which the reference mutates in place and its filters and callbacks read.  The
    aggregation hook that follows adopts the poisoned rows: nothing is staged twice.  Composes with the
    aggregation mixins by inheritance; on several ``aggregation_devices`` the attack runs on the first
    and always writes back.
    """

    #: None = ``Config().clients.attack_type`` / ``.per_round`` / ``.lambada_value``
    attack_simulation_type = None
    attack_per_round = None
    attack_lambada_value = None
    #: copy the poisoned rows back into the attackers' payload tensors (D2H); False for rounds whose
    #: payloads nothing reads between the attack and the aggregation on the device
    attack_writeback = True

    def _attack_setting(self, own: str, name: str):
        value = getattr(self, own)
        return value if value is not None else _clients_config(name)

    def weights_attacked(self, weights_received):
        from ..attacks import KINDS

        kind = KINDS.get(self._attack_setting("attack_simulation_type", "attack_type"))
        if kind is None:
            return super().weights_attacked(weights_received)
        at = [i for i, update in enumerate(self.updates) if update.client_id in self.attacker_list]
        if not at or (kind == "lie" and len(at) == 1):  # no attacker; "LIE attack does not apply to solo attacker"
            return weights_received
        payloads = [weights_received[i] for i in at]
        codec = payload_codec(payloads[0])
        if codec != "native":
            raise ValueError(f"the attack simulation takes native payloads, not {codec} codes")
        params = {}
        if kind == "lie":
            params["per_round"] = self._attack_setting("attack_per_round", "per_round")
        elif kind == "lambda":
            params["lambada_value"] = self._attack_setting("attack_lambada_value", "lambada_value")
        engine = self.aggregation_engine()
        multi = getattr(engine, "primary", None) is not None
        if multi:
            engine = engine.primary
        baseline = self.algorithm.extract_weights()
        rnd = engine.begin(baseline, len(payloads))
        rnd.deltas = False  # the rows stay weights: the deltas are formed in scratch
        rnd.put_baseline(baseline)
        with tracing.range("plato_amd.attack.stage"):
            in_arrival_rows = stage_as_arrivals(engine, rnd, payloads)
        with tracing.range("plato_amd.attack.launch"):
            rnd.launch_attack(kind, range(len(payloads)), **params)
        if self.attack_writeback or multi or not in_arrival_rows:
            with tracing.range("plato_amd.attack.writeback"):
                rows = rnd.fetch_rows(range(len(payloads)))
                for payload, (row_f, row_i) in zip(payloads, rows):
                    for name, src in rnd.layout.unpack(row_f, row_i).items():
                        payload[name].copy_(src)  # in place, as perform_model_poisoning
                    engine.refresh_arrival(payload)
        self._plato_amd_attack = dict(rnd.attack, timings=dict(rnd.timings))
        return weights_received


def _detector_type():
    """``Config().server.detector_type``, or None where it is not set or Plato is not installed."""
    try:
        from plato.config import Config
    except ImportError:
        return None
    return getattr(Config().server, "detector_type", None)


class DetectorFilterMixin(_EngineHolder):
    """``weights_filter`` of the detector server (detector_server.py:137-175) on the GPU for the defence
    "FLDetector" of ``server.detector_type`` (``detectors.fl_detector``); every other name and no defence
    at all go to the base class unchanged.

    The received payloads are staged as arrival rows (or adopted, where the attack simulation or the
    arrival hook staged them), scored there (``AggregationRound.launch_fldetector``) and the payloads that
    were not flagged are returned in order.  The aggregation hook that follows adopts their rows: nothing
    is staged twice.  The record is the engine's (``engine.fldetector``) and is kept across rounds.
    Composes with :class:`AttackSimulationMixin` and the aggregation mixins by inheritance.
    """

    #: None = ``Config().server.detector_type``
    detector_type = None

    def weights_filter(self, weights_attacked):
        from .. import _lib

        own = self.detector_type
        name = own if own is not None else _detector_type()
        if name != "FLDetector":
            return super().weights_filter(weights_attacked)
        codec = payload_codec(weights_attacked[0])
        if codec != "native":
            raise ValueError(f"the FLDetector defence takes native payloads, not {codec} codes")
        engine = self.aggregation_engine()
        if getattr(engine, "primary", None) is not None:
            raise NotImplementedError("the FLDetector defence runs on one GPU (aggregation_devices has several)")
        if len(weights_attacked) > _lib.PLATO_AGG_ROBUST_MAX_K:
            raise ValueError(f"the FLDetector defence takes at most {_lib.PLATO_AGG_ROBUST_MAX_K} clients, "
                             f"got {len(weights_attacked)}")
        baseline = self.algorithm.extract_weights()
        received_ids = [update.client_id for update in self.updates]
        rnd = engine.begin(baseline, len(weights_attacked))
        rnd.deltas = False  # the rows stay weights: the deltas are formed in registers
        rnd.put_baseline(baseline)
        with tracing.range("plato_amd.detector.stage"):
            stage_as_arrivals(engine, rnd, weights_attacked)
        with tracing.range("plato_amd.detector.launch"):
            rnd.launch_fldetector(received_ids)
        flagged = set(rnd.detector["malicious"])
        self._plato_amd_detector = dict(rnd.detector, timings=dict(rnd.timings))
        return [payload for i, payload in enumerate(weights_attacked) if i not in flagged]
