"""Sub-model aggregation hook: the width-heterogeneous servers of the reference's model-search examples.

``examples/model_search/{heterofl,fjord,fedrolex,anycostfl}/*_server.py`` define ``aggregate_weights`` as
``self.algorithm.aggregation(weights_received)``: every global element becomes the mean of the clients
whose leading-corner box covers it (``plato_amd.submodel``).  Here that runs on the GPU
(``plato_agg_submodel_mean``); the hooks around it (``customize_server_response``, ``weights_aggregated``
with its channel sorting and sBN, ``clients_processed``) are the base class's, unchanged::

    Server = make_server(base=heterofl_server.Server, mixin=SubmodelAggregationMixin)

HeteroFL and FjORD take ``submodel_rule = "heterofl"`` (the default), FedRolex and AnyCostFL
``"fedrolex"`` (a 3-D entry is boxed on its three dims).  ``sysheterofl`` is another rule, under names of its own:
``plato_amd.servers.elastic``.
"""

from __future__ import annotations

from .. import tracing
from .fedavg import _EngineHolder


class _BoxAggregationMixin(_EngineHolder):
    """``aggregate_weights`` hook of the model-search servers, on one GPU: a kind names itself and begins
    its round (``plato_amd.servers.elastic`` has the other one)."""

    _kind: str

    def _begin_round(self, engine, state_dict, weights_received):
        raise NotImplementedError

    async def aggregate_weights(self, updates, baseline_weights, weights_received):
        # baseline_weights is not read: the reference aggregates on top of algorithm.model's state_dict
        engine = self.aggregation_engine()
        if getattr(engine, "primary", None) is not None:
            raise NotImplementedError(f"{self._kind} aggregation runs on one GPU (aggregation_devices has several)")
        try:
            rnd = self._begin_round(engine, self.algorithm.model.state_dict(), weights_received)

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


class SubmodelAggregationMixin(_BoxAggregationMixin):
    """``aggregate_weights`` hook of the sub-model servers, on one GPU."""

    #: "heterofl" (HeteroFL, FjORD) or "fedrolex" (FedRolex, AnyCostFL): plato_amd.submodel.RULES
    submodel_rule = "heterofl"
    _kind = "sub-model"

    def _begin_round(self, engine, state_dict, weights_received):
        return engine.begin_submodels(state_dict, weights_received, self.submodel_rule)
