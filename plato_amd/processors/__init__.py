"""Server processors whose work runs natively.

Inbound:

* ``qsgd``: QSGD payloads stay coded to HBM, decoded in the FedAvg kernel.
* ``zstd``: model_compress payloads decompressed and parsed natively into pinned arenas.

Outbound:

* ``prune``: the reference's ``unstructured_pruning`` (global magnitude pruning), selected and masked on
  the device; ``UnstructuredPruning`` is its ``Processor``.
* ``qsgd_encode``: the reference's ``model_quantize_qsgd`` (QSGD quantizer), the maxima and the stochastic
  rounding on the device; ``QsgdQuantize`` is its ``Processor``.  ``qsgd`` decodes what it produces.
"""

from . import prune, qsgd_encode  # noqa: F401
from .prune import Processor as UnstructuredPruning  # noqa: F401
from .qsgd import QsgdPayload  # noqa: F401
from .qsgd_encode import Processor as QsgdQuantize  # noqa: F401
