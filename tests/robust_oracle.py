"""CPU restatement of plato_agg_robust_columns (include/plato_agg.h): numpy, exactly the kernel's semantics.

The checker for shapes with no reference fixture.  ``x_f32``: [K, n] float32; ``x_i64``: [K, m] int64
(promoted to float32 with round to nearest even, as ``flatten_weights``' torch.cat does).
"""

from __future__ import annotations

import numpy as np

CANON_NAN = np.uint32(0x7FC00000)


def sort_keys(x: np.ndarray) -> np.ndarray:
    """Order-preserving uint32 keys of float32 values: the total order with -0 < +0."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u >> np.uint32(31), ~u, u | np.uint32(0x80000000))


def from_keys(k: np.ndarray) -> np.ndarray:
    u = np.where(k >> np.uint32(31), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    return u.view(np.float32)


def median_columns(x: np.ndarray) -> np.ndarray:
    """Lower median per column of a [K, n] matrix; NaN (canonical) where the column holds a NaN."""
    x = np.ascontiguousarray(x)
    if x.dtype == np.int64:
        x = x.astype(np.float32)  # RNE
    assert x.dtype == np.float32 and x.ndim == 2 and x.shape[0] >= 1
    k = x.shape[0]
    keys = np.sort(sort_keys(x), axis=0)
    out = from_keys(keys[(k - 1) // 2]).copy()
    out.view(np.uint32)[np.isnan(x).any(axis=0)] = CANON_NAN
    return out


def median(x_f32: np.ndarray, x_i64: np.ndarray):
    """(fp32 region, int64 region as fp32) of the coordinate-wise median."""
    k = x_f32.shape[0]
    out_i = median_columns(x_i64) if x_i64.size else np.zeros(0, dtype=np.float32)
    out_f = median_columns(x_f32) if x_f32.size else np.zeros(0, dtype=np.float32)
    assert x_i64.shape[0] == k or not x_i64.size
    return out_f, out_i
