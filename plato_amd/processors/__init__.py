"""Server processors whose work runs natively.

Inbound:

* ``qsgd``: QSGD payloads stay coded to HBM, decoded in the FedAvg kernel.
* ``zstd``: model_compress payloads decompressed and parsed natively into pinned arenas.

Outbound:

* ``prune``: the reference's ``unstructured_pruning`` (global magnitude pruning), selected and masked on
  the device; ``UnstructuredPruning`` is its ``Processor``.
"""

from . import prune  # noqa: F401
from .prune import Processor as UnstructuredPruning  # noqa: F401
from .qsgd import QsgdPayload  # noqa: F401
