"""TEST INFRASTRUCTURE ONLY — the QSGD quantizer restated with numpy (include/plato_agg.h,
plato_agg_qsgd_encode; the reference is plato/processors/model_quantize_qsgd.py: Processor._process_layer).

Every operation is one fp32 numpy operation, so every rounding is the reference's.  The draws are the
project's counter generator (oracle/synth.py): element i of a row gets 24 bits of
``splitmix64(synth_key(seed, 0x51534744) + (i >> 1))``, the high ones for an even i.  The fixtures
(tests/golden/make_golden_qsgd_encode.py) were made by feeding these draws to the reference's own code.
"""

from __future__ import annotations

import struct
from collections import OrderedDict

import numpy as np

from oracle import synth

DRAW_STREAM = 0x51534744
_U64 = np.uint64


def draws(seed: int, start: int, n: int) -> np.ndarray:
    """u of the row elements [start, start + n): fp32 multiples of 2^-24 in [0, 1)."""
    key = _U64(synth.synth_key(seed & synth._MASK, DRAW_STREAM))
    i = np.arange(start, start + n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (i >> _U64(1)) + key
        z = z + synth._GOLD
        z = (z ^ (z >> _U64(30))) * synth._M1
        z = (z ^ (z >> _U64(27))) * synth._M2
        h = z ^ (z >> _U64(31))
    shift = np.where(i & _U64(1) == 0, _U64(40), _U64(16))
    bits = ((h >> shift) & _U64(0xFFFFFF)).astype(np.uint32)
    return bits.astype(np.float32) * np.float32(2.0**-24)


def max_key(values: np.ndarray) -> int:
    """max of bits & 0x7fffffff over fp32 values (0 for none)."""
    bits = np.ascontiguousarray(values, dtype=np.float32).reshape(-1).view(np.uint32)
    return int((bits & np.uint32(0x7FFFFFFF)).max()) if bits.size else 0


def encode_values(values: np.ndarray, level: int, u: np.ndarray) -> tuple[np.ndarray, int]:
    """(codes, max key) of one flattened fp32 entry under the draws ``u``.  An all-zero entry gives zero
    codes; the codes of a non-finite entry mean nothing."""
    v = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
    key = max_key(v)
    if key == 0:
        return np.zeros(v.size, dtype=np.uint8), key
    m = np.array([key], dtype=np.uint32).view(np.float32)[0]
    tp = np.float32(level - 1)
    with np.errstate(all="ignore"):
        ratio = np.divide(np.abs(v), m, dtype=np.float32)
        x = np.multiply(ratio, tp, dtype=np.float32)
        lvl = np.ceil(np.subtract(x, np.float32(1), dtype=np.float32))
        p = np.subtract(x, lvl, dtype=np.float32)
        if key >= 0x7F800000:
            return np.zeros(v.size, dtype=np.uint8), key
        mag = lvl.astype(np.int64) + (u.astype(np.float32) <= p)
    negative = (v < 0) & (mag > 0)
    return (mag | np.where(negative, 0x80, 0)).astype(np.uint8), key


def header(key: int, shape) -> bytes:
    """!f m | !I numel | !h ndim | ndim x !h dim, m given by its bits."""
    out = struct.pack("!I", key) + struct.pack("!I", int(np.prod(shape, dtype=np.int64))) + struct.pack("!h", len(shape))
    for dim in shape:
        out += struct.pack("!h", int(dim))
    return out


def as_f32(a: np.ndarray) -> np.ndarray:
    """An entry as the fp32 values that are quantized: an int64 entry is converted, round to nearest even."""
    return a.astype(np.float32) if a.dtype == np.int64 else np.ascontiguousarray(a, dtype=np.float32)


def encode_state(state, level: int, seed: int) -> "OrderedDict[str, bytes]":
    """name -> wire bytes of a state (name -> numpy array, fp32 or int64) whose entries are staged one after
    the other into one row, in order: the entry at row offset ``at`` takes the draws [at, at + numel)."""
    out, at = OrderedDict(), 0
    for name, a in state.items():
        v = as_f32(np.asarray(a)).reshape(-1)
        codes, key = encode_values(v, level, draws(seed, at, v.size))
        out[name] = header(key, np.asarray(a).shape) + codes.tobytes()
        at += v.size
    return out


def encode_row(row_bits: np.ndarray, pieces, level: int, seed: int, codes: np.ndarray):
    """What plato_agg_qsgd_encode leaves: ``codes`` (a copy) with the pieces' bytes replaced, and the keys."""
    values = row_bits.view(np.float32)
    out = codes.copy()
    keys = np.zeros(len(pieces), dtype=np.uint32)
    for p, (b, e) in enumerate(pieces):
        if e > b:
            out[b:e], keys[p] = encode_values(values[b:e], level, draws(seed, b, e - b))
    return out, keys
