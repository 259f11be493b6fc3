"""Elastic sub-model aggregation hook: the depth- and width-heterogeneous server of the reference's
model-search examples.

``examples/model_search/sysheterofl/sysheterofl_server.py`` defines ``aggregate_weights`` as
``self.algorithm.aggregation(weights_received)``: every global element becomes the mean of the clients that
hold its key and whose leading-corner box covers it (``plato_amd.elastic``).  Here that runs on the GPU
(``plato_agg_elastic_mean``); the hooks around it (``customize_server_response`` with the architecture
search, ``clients_processed`` with its distillation, ``training_will_start``) are the base class's,
unchanged::

    Server = make_server(base=sysheterofl_server.Server, mixin=ElasticAggregationMixin)

The reference's ``distillation()`` calls ``aggregation(..., update_track=False)`` and discards the result;
the engine takes the flag (``FedAvgEngine.aggregate_elastic``), nothing here passes it.
"""

from __future__ import annotations

from .. import tracing
from .fedavg import _EngineHolder


class ElasticAggregationMixin(_EngineHolder):
    """``aggregate_weights`` hook of the sysheterofl server, on one GPU."""

    async def aggregate_weights(self, updates, baseline_weights, weights_received):
        # baseline_weights is not read: the reference aggregates on top of algorithm.model's state_dict
        engine = self.aggregation_engine()
        if getattr(engine, "primary", None) is not None:
            raise NotImplementedError("elastic aggregation runs on one GPU (aggregation_devices has several)")
        try:
            rnd = engine.begin_elastic(self.algorithm.model.state_dict(), weights_received)

            def stage():
                with tracing.range("plato_amd.stage"):
                    rnd.stage()

            await self._off_loop(stage)
            with tracing.range("plato_amd.launch"):
                rnd.launch()
            with tracing.range("plato_amd.fetch"):
                return await self._finish(rnd)
        finally:
            # payloads of the full model may have been staged at arrival: their slots go back unused
            engine.release_arrivals()
