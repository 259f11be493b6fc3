"""Drop-in for the reference's ``unstructured_pruning`` processor (plato/processors/unstructured_pruning.py):
global magnitude pruning of ``trainer.model``, the selection and the masked write on the device
(``plato_amd.prune``).
"""

from __future__ import annotations

import logging
from typing import Any

import torch.nn.utils.prune as prune

from ..prune import prunable_weights, prune_model


class Processor:
    """Same constructor arguments and ``process`` as the reference's: ``process(data)`` ignores ``data``,
    prunes ``trainer.model`` in place and returns ``model.cpu().state_dict()``.  The selection runs on every
    call; nothing is cached between calls."""

    def __init__(self, parameters_to_prune=None, pruning_method=prune.L1Unstructured, amount=0.2, name=None,
                 trainer=None, client_id=None, server_id=None, device="cuda:0", **kwargs) -> None:
        if pruning_method is not prune.L1Unstructured:
            raise NotImplementedError(
                "plato_amd unstructured_pruning: only prune.L1Unstructured runs on the device "
                f"(got {getattr(pruning_method, '__name__', pruning_method)!r})")
        self.name = name
        self.trainer = trainer
        self.client_id = client_id
        self.server_id = server_id
        self.parameters_to_prune = parameters_to_prune
        self.pruning_method = pruning_method
        self.amount = amount
        self.device = device
        self.model = None
        self.last_result = None

    def process(self, data: Any) -> Any:
        self.model = self.trainer.model
        if self.parameters_to_prune is None:
            self.parameters_to_prune = prunable_weights(self.model)
        self.last_result = prune_model(self.model, self.amount, self.parameters_to_prune, self.device)
        output = self.model.cpu().state_dict()
        if self.client_id is None:
            logging.info("[Server #%d] Global unstructured pruning applied.", self.server_id)
        else:
            logging.info("[Client #%d] Global unstructured pruning applied.", self.client_id)
        return output

    def process_iterable(self, data):
        return map(self.process, data)

    def __repr__(self) -> str:
        return self.name
