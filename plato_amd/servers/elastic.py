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

from .submodel import _BoxAggregationMixin


class ElasticAggregationMixin(_BoxAggregationMixin):
    """``aggregate_weights`` hook of the sysheterofl server, on one GPU."""

    _kind = "elastic"

    def _begin_round(self, engine, state_dict, weights_received):
        return engine.begin_elastic(state_dict, weights_received)
