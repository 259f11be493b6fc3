"""Drop-in for the reference's ``model_quantize_qsgd`` processor (plato/processors/model_quantize_qsgd.py):
every entry of the payload quantized with QSGD, the maxima and the stochastic rounding on the device
(``plato_amd.qsgd_encode``).
"""

from __future__ import annotations

import logging
import os
import pickle
import sys
from typing import Any

from ..qsgd_encode import check_level, encode_state_dict

_MASK = (1 << 64) - 1


def splitmix64(z: int) -> int:
    """The project's counter generator (include/plato_agg.h, plato_agg_fill_synth_*)."""
    z = (z + 0x9E3779B97F4A7C15) & _MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK
    return z ^ (z >> 31)


class Processor:
    """Same constructor arguments and ``process`` as the reference's: ``process(data)`` returns an
    ``OrderedDict`` name -> bytes in ``data``'s key order, which ``model_dequantize_qsgd`` (or
    ``plato_amd.processors.qsgd.Processor``) decodes.

    The reference seeds its draws from the OS on every entry.  ``seed=None`` does the same once per call: 64
    fresh bits from ``os.urandom``.  An integer ``seed`` makes the bytes reproducible: call number c (0 for
    the first ``process``) uses ``splitmix64(seed + c)``.  The seed a call used is kept as ``last_seed``."""

    def __init__(self, quantization_level=64, client_id=None, server_id=None, seed=None, device="cuda:0",
                 **kwargs) -> None:
        self.quantization_level = check_level(quantization_level)
        self.client_id = client_id
        self.server_id = server_id
        if seed is not None and (isinstance(seed, bool) or not isinstance(seed, int)):
            raise TypeError(f"seed={seed!r} must be None or an integer")
        self.seed = seed
        self.device = device
        self.calls = 0
        self.last_seed = None

    def next_seed(self) -> int:
        """The seed of the next call; counts the call."""
        if self.seed is None:
            seed = int.from_bytes(os.urandom(8), "little")
        else:
            seed = splitmix64((self.seed + self.calls) & _MASK)
        self.calls += 1
        return seed

    def process(self, data: Any) -> Any:
        seed = self.next_seed()
        new_data = encode_state_dict(data, self.quantization_level, seed, self.device)
        self.last_seed = seed
        if logging.getLogger().isEnabledFor(logging.INFO):  # the sizes cost two pickles of the model
            old_size = sys.getsizeof(pickle.dumps(data))
            new_size = sys.getsizeof(pickle.dumps(new_data))
            if self.client_id is None:
                logging.info("[Server #%d] Processed the model and changed its size from %.2f MB to %.2f MB.",
                             self.server_id, old_size / 1024**2, new_size / 1024**2)
            else:
                logging.info("[Client #%d] Processed the model and changed its size from %.2f MB to %.2f MB.",
                             self.client_id, old_size / 1024**2, new_size / 1024**2)
        return new_data

    def process_iterable(self, data):
        return map(self.process, data)
