"""Numpy restatement of plato_agg_prune_global (include/plato_agg.h): the keys bits & 0x7fffffff, a stable
argsort (lowest flat index first among equal keys), and w * 0.0f formed from the bits."""

from __future__ import annotations

import numpy as np


def keys(bits: np.ndarray) -> np.ndarray:
    return bits.astype(np.uint32) & np.uint32(0x7FFFFFFF)


def times_zero(bits: np.ndarray) -> np.ndarray:
    """w * 0.0f as x86-64 evaluates it: the sign for a finite w, the quieted NaN, 0xffc00000 for +-inf."""
    bits = bits.astype(np.uint32)
    k = keys(bits)
    out = bits & np.uint32(0x80000000)
    out = np.where(k == 0x7F800000, np.uint32(0xFFC00000), out)
    out = np.where(k > 0x7F800000, bits | np.uint32(0x00400000), out)
    return out.astype(np.uint32)


def prune_flat(bits: np.ndarray, k: int):
    """The pruned bits of the flat vector and the record (T, #(key < T), #(key == T), r)."""
    bits = np.ascontiguousarray(bits, dtype=np.uint32)
    n = bits.size
    if not 0 <= k <= n:
        raise ValueError("k out of range")
    if k == 0:
        return bits.copy(), (0, 0, 0, 0)
    ky = keys(bits)
    order = np.argsort(ky, kind="stable")
    t = int(ky[order[k - 1]])
    below = int(np.count_nonzero(ky < t))
    ties = int(np.count_nonzero(ky == t))
    out = bits.copy()
    chosen = order[:k]
    out[chosen] = times_zero(bits[chosen])
    return out, (t, below, ties, k - below)


def prune_row(row_bits: np.ndarray, pieces, k: int):
    """The row with its pieces ([begin, end) element ranges, in table order) pruned; the rest untouched."""
    row_bits = np.ascontiguousarray(row_bits, dtype=np.uint32)
    idx = np.concatenate([np.arange(b, e, dtype=np.int64) for b, e in pieces] + [np.zeros(0, dtype=np.int64)])
    flat, record = prune_flat(row_bits[idx], k)
    out = row_bits.copy()
    out[idx] = flat
    return out, record
