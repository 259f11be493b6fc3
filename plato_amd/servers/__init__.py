"""Server-side plugin surface: GPU-backed aggregation hooks for Plato servers."""

from .fedavg import DeltasAggregationMixin, FusedAggregationMixin, make_server  # noqa: F401
from .ingest import WireIngestMixin  # noqa: F401
from .robust import (AttackSimulationMixin, DetectorAggregationMixin, DetectorFilterMixin,  # noqa: F401
                     RobustAggregationMixin, TrustAggregationMixin)
from .elastic import ElasticAggregationMixin  # noqa: F401
from .submodel import SubmodelAggregationMixin  # noqa: F401
