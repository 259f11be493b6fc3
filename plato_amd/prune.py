"""Global magnitude pruning on the device: the reference's ``unstructured_pruning`` outbound processor.

``torch.nn.utils.prune.global_unstructured(parameters, L1Unstructured, amount)`` followed by
``prune.remove`` zeroes, of all prunable weights together, the k with the smallest magnitude.  Here the
prunable weights are staged into one fp32 device row, ``plato_agg_prune_global`` (``csrc/prune.hip``,
DESIGN.md §26) finds the threshold by a radix select and writes the masked row, and the weights are copied
back into the parameters in place.  The host keeps what is small: the prunable set and its order, the count
k with the reference's rounding and errors, and the re-registration that gives ``state_dict()`` the
reference's key order.
"""

from __future__ import annotations

import numbers
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib

#: what one workgroup consumes per grid step, and the grid of a streaming launch (csrc/prune.hip)
TILE = _lib.PLATO_AGG_PRUNE_TILE
GRID = _lib.PLATO_AGG_PRUNE_GRID


@dataclass(frozen=True)
class PruneResult:
    """What ``plato_agg_prune_global`` did: the threshold key T = bits & 0x7fffffff of rank k - 1, the number
    of keys below it, the number equal to it, and how many of those were pruned (the lowest flat indices)."""

    k: int
    threshold_key: int
    below: int
    ties: int
    ties_pruned: int

    @property
    def threshold(self) -> float:
        """|w| at the threshold."""
        return float(np.array([self.threshold_key], dtype=np.uint32).view(np.float32)[0])


def prunable_weights(model: torch.nn.Module) -> list[tuple[torch.nn.Module, str]]:
    """The reference's default ``parameters_to_prune``: the ``weight`` of every ``Conv2d`` and ``Linear``
    in ``named_modules()`` order (unstructured_pruning.py:37-42)."""
    return [(module, "weight") for _, module in model.named_modules()
            if isinstance(module, (torch.nn.Conv2d, torch.nn.Linear))]


def nparams_toprune(amount, n: int) -> int:
    """k for ``amount`` of ``n`` elements, with torch.nn.utils.prune's checks and rounding
    (``_validate_pruning_amount_init``, ``_compute_nparams_toprune``, ``_validate_pruning_amount``): an
    integral amount is k itself, a float amount gives Python's ``round(amount * n)``."""
    if not isinstance(amount, numbers.Real):
        raise TypeError(f"Invalid type for amount: {amount}. Must be int or float.")
    if (isinstance(amount, numbers.Integral) and amount < 0) or (
            not isinstance(amount, numbers.Integral) and (float(amount) > 1.0 or float(amount) < 0.0)):
        raise ValueError(f"amount={amount} should either be a float in the range [0, 1] or a non-negative integer")
    k = int(amount) if isinstance(amount, numbers.Integral) else round(amount * n)
    if isinstance(amount, numbers.Integral) and amount > n:
        raise ValueError(f"amount={amount} should be smaller than the number of parameters to prune={n}")
    return k


def piece_table(pieces) -> np.ndarray:
    """``plato_agg_chunk`` rows (entry, begin, end, reserved) for [begin, end) element ranges of a row."""
    table = np.zeros((len(pieces), 4), dtype=np.uint32)
    for p, (begin, end) in enumerate(pieces):
        if not (0 <= begin <= _lib.PLATO_AGG_PRUNE_MAX_ELEMENTS and 0 <= end <= _lib.PLATO_AGG_PRUNE_MAX_ELEMENTS):
            raise ValueError("plato_agg_prune_global: a piece lies outside a row of 2^32 - 1 elements")
        table[p] = (p, begin, end, 0)
    return table


def prune_row(row: torch.Tensor, pieces, k: int) -> PruneResult:
    """Prune in place the k smallest-magnitude elements of the ``pieces`` ([begin, end) element ranges,
    ascending and disjoint) of a contiguous fp32 device row; everything else keeps its bits."""
    if row.dtype != torch.float32 or not row.is_contiguous() or row.dim() != 1:
        raise ValueError("prune_row: the row must be a contiguous 1-d float32 tensor")
    if not row.is_cuda:
        raise RuntimeError("prune_row: the row must be on the GPU (there is no host path)")
    table = piece_table(pieces)
    n = int(sum(int(e) - int(b) for b, e in pieces if e > b))
    k = int(k)
    if k < 0:
        raise ValueError("prune_row: k must not be negative")
    lib = _lib.lib()
    size = lib.plato_agg_prune_global_workspace(len(table), n)
    if size == 0:
        raise ValueError("plato_agg_prune_global: more than 2^20 pieces or 2^32 - 1 elements")
    with torch.cuda.device(row.device):
        stream = torch.cuda.current_stream(row.device)
        workspace = torch.empty(size, dtype=torch.uint8, device=row.device)
        result = torch.zeros(4, dtype=torch.int64, device=row.device)
        _lib.call("plato_agg_prune_global", row.data_ptr(), row.numel(), table.ctypes.data, len(table), k,
                  workspace.data_ptr(), result.data_ptr(), stream.cuda_stream)
        # the fetch also keeps `table` alive until the stream has uploaded it
        t, below, ties, r = (int(v) for v in result.cpu().tolist())
    return PruneResult(k=k, threshold_key=t, below=below, ties=ties, ties_pruned=r)


def stage_row(tensors, device) -> tuple[torch.Tensor, list[tuple[int, int]]]:
    """The tensors flattened one after the other into one fp32 device row, and their pieces."""
    pieces, at = [], 0
    for t in tensors:
        pieces.append((at, at + t.numel()))
        at += t.numel()
    row = torch.empty(at, dtype=torch.float32, device=device)
    for t, (b, e) in zip(tensors, pieces):
        row[b:e].copy_(t.detach().reshape(-1))
    return row, pieces


def prune_model(model: torch.nn.Module, amount=0.2, parameters_to_prune=None, device="cuda:0") -> PruneResult:
    """``prune.global_unstructured(parameters_to_prune, L1Unstructured, amount)`` and ``prune.remove`` of
    every pruned parameter, on the device: the parameters' data are overwritten in place, and each pruned
    parameter is re-registered last in its module's ``_parameters`` (what ``prune.remove`` leaves behind:
    ``state_dict()`` lists ``bias`` before ``weight`` from then on)."""
    if parameters_to_prune is None:
        parameters_to_prune = prunable_weights(model)
    params = [getattr(module, name) for module, name in parameters_to_prune]
    for p in params:
        if p.dtype != torch.float32:
            raise NotImplementedError("prune_model: only float32 parameters are supported")
    n = sum(p.numel() for p in params)
    k = nparams_toprune(amount, n)
    if k > n:  # a float amount cannot get here; kept beside the reference's check
        raise ValueError(f"amount={amount} should be smaller than the number of parameters to prune={n}")
    device = torch.device(device)
    if k:
        row, pieces = stage_row(params, device)
        result = prune_row(row, pieces, k)
        with torch.no_grad():
            for p, (b, e) in zip(params, pieces):
                p.data.copy_(row[b:e].reshape(p.shape))
    else:
        result = PruneResult(k=0, threshold_key=0, below=0, ties=0, ties_pruned=0)
    for module, name in parameters_to_prune:
        param = module._parameters.pop(name)
        module._parameters[name] = param
    return result
