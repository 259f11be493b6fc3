"""The QSGD quantizer on the device: the reference's ``model_quantize_qsgd`` outbound processor.

``Processor._process_layer`` (plato/processors/model_quantize_qsgd.py) turns every entry of a state_dict into
its maximum magnitude and one stochastically rounded byte per element, in two Python loops over the elements.
Here the entries are staged into one fp32 device row, ``plato_agg_qsgd_encode`` (``csrc/qsgd_encode.hip``,
DESIGN.md §27) finds the maxima and writes the codes, one D2H copy fetches both, and the host packs each
entry's header in front of its slice of the codes.  ``plato_amd.processors.qsgd`` and
``plato_agg_fedavg_qsgd`` are the decoder of this wire format.

The reference draws from ``random.seed()`` (OS entropy); its bytes are not reproducible.  Here the draw of a
row element is a function of ``(seed, row index)`` alone (include/plato_agg.h), so a seed reproduces the
bytes.  Two documented differences: an all-zero entry is encoded as ``m = 0`` with zero codes (the reference
raises ``struct.error``; its dequantizer turns this back into zeros), and a non-finite entry raises
``ValueError`` naming the entry (the reference raises ``struct.error``).
"""

from __future__ import annotations

import struct
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from .prune import piece_table

#: what one workgroup consumes per grid step, and the grid of a streaming launch (csrc/qsgd_encode.hip)
TILE = _lib.PLATO_AGG_QSGD_ENCODE_TILE
GRID = _lib.PLATO_AGG_QSGD_ENCODE_GRID
MAX_DIM = 32767          # the header's "!h"
MAX_NUMEL = (1 << 32) - 1  # the header's "!I"
_MASK = (1 << 64) - 1
_FIRST_NONFINITE = 0x7F800000


def check_level(level) -> int:
    if isinstance(level, bool) or not isinstance(level, (int, np.integer)) or not 2 <= int(level) <= 128:
        raise ValueError(f"quantization_level={level!r} must be an integer in [2, 128] (one byte: 7 bits and a sign)")
    return int(level)


def _round4(n: int) -> int:
    return (n + 3) & ~3


def _encode_into(row: torch.Tensor, pieces, level: int, seed: int, codes: torch.Tensor, keys: torch.Tensor):
    """Codes into ``codes`` (row.numel() bytes), maxima into ``keys`` (4 bytes per piece), on the current
    stream.  Returns the host table, which the stream uploads: the caller keeps it until the stream is there."""
    table = piece_table(pieces)
    n = int(sum(int(e) - int(b) for b, e in pieces if e > b))
    lib = _lib.lib()
    size = lib.plato_agg_qsgd_encode_workspace(len(table), n)
    if size == 0:
        raise ValueError("plato_agg_qsgd_encode: more than 2^20 pieces or 2^32 - 1 elements")
    with torch.cuda.device(row.device):
        stream = torch.cuda.current_stream(row.device)
        workspace = torch.empty(size, dtype=torch.uint8, device=row.device)
        if n == 0:  # the call launches nothing and writes nothing
            keys.zero_()
        _lib.call("plato_agg_qsgd_encode", row.data_ptr(), row.numel(), table.ctypes.data, len(table), level,
                  seed & _MASK, codes.data_ptr(), keys.data_ptr(), workspace.data_ptr(), stream.cuda_stream)
    return table


def encode_row(row: torch.Tensor, pieces, level: int, seed: int, codes: torch.Tensor | None = None):
    """QSGD codes of the ``pieces`` ([begin, end) element ranges, ascending and disjoint; one per entry) of a
    contiguous fp32 device row.  Returns ``(codes, max_keys)``, both on the device: ``codes[i]`` (uint8) is the
    code of ``row[i]``, ``max_keys[p]`` (int32) the bits of piece p's maximum magnitude (0: all zero or empty;
    >= 0x7f800000 as unsigned: the piece holds an infinity or a NaN and its codes mean nothing).  With
    ``codes`` given (a contiguous uint8 device tensor of ``row.numel()`` bytes, 4-byte aligned) the codes are
    written into it and its bytes outside the pieces keep their value; a fresh one is zero there."""
    if row.dtype != torch.float32 or not row.is_contiguous() or row.dim() != 1:
        raise ValueError("encode_row: the row must be a contiguous 1-d float32 tensor")
    if not row.is_cuda:
        raise RuntimeError("encode_row: the row must be on the GPU (there is no host path)")
    level = check_level(level)
    n_row, n_pieces = row.numel(), len(pieces)
    if codes is None:
        codes = torch.zeros(n_row, dtype=torch.uint8, device=row.device)
    elif (codes.dtype != torch.uint8 or not codes.is_contiguous() or codes.dim() != 1 or codes.numel() != n_row
          or codes.device != row.device):
        raise ValueError("encode_row: codes must be a contiguous uint8 tensor of the row's length on its device")
    keys = torch.zeros(n_pieces, dtype=torch.int32, device=row.device)
    table = _encode_into(row, pieces, level, int(seed), codes, keys)
    torch.cuda.current_stream(row.device).synchronize()  # the stream has read `table`
    del table
    return codes, keys


def header(max_key: int, shape) -> bytes:
    """``!f m | !I numel | !h ndim | ndim x !h dim`` (model_quantize_qsgd.py:71-76), m given by its bits."""
    numel = 1
    for dim in shape:
        numel *= int(dim)
    return struct.pack(f"!IIh{len(shape)}h", max_key, numel, len(shape), *(int(d) for d in shape))


def _check_entries(state_dict) -> None:
    for name, t in state_dict.items():
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"encode_state_dict: entry {name!r} is not a tensor")
        if t.dtype not in (torch.float32, torch.int64):
            raise NotImplementedError(f"encode_state_dict: entry {name!r} is {t.dtype}; only float32 and int64 "
                                      "entries are supported")
        if any(d > MAX_DIM for d in t.shape):
            raise ValueError(f"encode_state_dict: entry {name!r} has a dimension above {MAX_DIM} "
                             f"(shape {tuple(t.shape)}); the wire header holds 16-bit sizes")
        if t.numel() > MAX_NUMEL:
            raise ValueError(f"encode_state_dict: entry {name!r} has 2^32 elements or more")


def encode_state_dict(state_dict, level: int = 64, seed: int = 0, device="cuda:0") -> "OrderedDict[str, bytes]":
    """``name -> bytes`` in the state_dict's key order, each value what the reference's ``_process_layer``
    returns for that entry under the draws of ``seed``: the entries are staged one after the other into one
    fp32 row on ``device`` (an int64 entry as fp32, which the reference's true division does to it as well),
    and entry number e at row offset ``at`` takes the draws of the row elements [at, at + numel)."""
    level = check_level(level)
    _check_entries(state_dict)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("encode_state_dict: the device must be a GPU (there is no host path)")
    names = list(state_dict)
    pieces, at = [], 0
    for name in names:
        n = state_dict[name].numel()
        pieces.append((at, at + n))
        at += n
    if at > MAX_NUMEL:
        raise ValueError("encode_state_dict: the state_dict has 2^32 elements or more")
    out = OrderedDict()
    if not names:
        return out
    tensors = [state_dict[name].detach() for name in names]
    with torch.cuda.device(device):
        if all(t.device.type == "cpu" for t in tensors):  # one pinned row, one H2D copy
            staged = torch.empty(at, dtype=torch.float32, pin_memory=True)
            target = staged
        else:
            staged = None
            target = torch.empty(at, dtype=torch.float32, device=device)
        for t, (b, e) in zip(tensors, pieces):
            if e > b:
                target[b:e].copy_(t.reshape(-1))  # int64 -> fp32: round to nearest even
        row = target if staged is None else staged.to(device, non_blocking=True)
        keys_at = _round4(at)
        buf = torch.empty(keys_at + 4 * len(names), dtype=torch.uint8, device=device)
        table = _encode_into(row, pieces, level, int(seed), buf[:at], buf[keys_at:])
        host = torch.empty(buf.numel(), dtype=torch.uint8, pin_memory=True)
        host.copy_(buf)  # the one D2H copy: codes and maxima; the stream has read `table` after it
        del table, staged
    raw = host.numpy()
    keys = raw[keys_at:].view(np.uint32)
    for name, key in zip(names, keys):
        if key >= _FIRST_NONFINITE:
            raise ValueError(f"encode_state_dict: entry {name!r} holds an infinity or a NaN")
    for name, key, (b, e) in zip(names, keys, pieces):
        out[name] = header(int(key), state_dict[name].shape) + raw[b:e].tobytes()
    return out
