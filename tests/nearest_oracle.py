"""CPU restatement of the nearest-mean mode of plato_agg_robust_columns (include/plato_agg.h) and of the
reference's Bulyan selection (examples/detector/aggregations.py:86-123): numpy only.

Per column c of the [K, n] matrix, with b = K - 2 * trim:
  1. an int64 column is promoted to float32, round to nearest even;
  2. a NaN anywhere in the column gives the canonical NaN 0x7fc00000;
  3. med = the lower median (robust_oracle.median_columns: total order, -0 < +0);
  4. d_k = |c_k - med|: one fp32 subtraction, sign bit cleared, a NaN distance replaced by 0x7fc00000;
     the unsigned bit pattern of d_k is its key;
  5. T = the key of rank b - 1; the rows with key < T are kept, then the rows with key == T in table
     order until b rows are kept (a stable sort of the keys and its first b rows);
  6. acc = +0; acc = fp32(acc + c_k) over the kept rows in table order; out = fp32(acc / fp32(b)).
"""

from __future__ import annotations

import numpy as np

from tests import krum_oracle as ko
from tests import robust_oracle as ro

CANON_NAN = ro.CANON_NAN


def _f32(x: np.ndarray) -> np.ndarray:
    x = np.ascontiguousarray(x)
    if x.dtype == np.int64:
        x = x.astype(np.float32)  # RNE
    assert x.dtype == np.float32 and x.ndim == 2 and x.shape[0] >= 1
    return x


def distance_keys(x: np.ndarray) -> np.ndarray:
    """[K, n] uint32: the sort keys of |x - lower median| (rule 4)."""
    x = _f32(x)
    med = ro.median_columns(x)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (x - med[None, :]).astype(np.float32)
    key = d.view(np.uint32) & np.uint32(0x7FFFFFFF)
    key[key > np.uint32(0x7F800000)] = CANON_NAN
    return key


def kept_rows(x: np.ndarray, trim: int) -> np.ndarray:
    """[K, n] bool: the rows each column keeps (rule 5)."""
    x = _f32(x)
    k = x.shape[0]
    assert 0 <= 2 * trim < k
    order = np.argsort(distance_keys(x), axis=0, kind="stable")  # equal keys: lowest table position first
    mask = np.zeros(x.shape, dtype=bool)
    np.put_along_axis(mask, order[: k - 2 * trim], True, axis=0)
    return mask


def nearest_mean_columns(x: np.ndarray, trim: int) -> np.ndarray:
    x = _f32(x)
    k = x.shape[0]
    mask = kept_rows(x, trim)
    acc = np.zeros(x.shape[1], dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(k):
            acc = np.where(mask[r], (acc + x[r]).astype(np.float32), acc)
        out = (acc / np.float32(k - 2 * trim)).astype(np.float32)
    out.view(np.uint32)[np.isnan(x).any(axis=0)] = CANON_NAN
    return out


def nearest_mean(x_f32: np.ndarray, x_i64: np.ndarray, trim: int):
    """(fp32 region, int64 region as fp32) of the nearest-mean mode."""
    out_f = nearest_mean_columns(x_f32, trim) if x_f32.size else np.zeros(0, dtype=np.float32)
    out_i = nearest_mean_columns(x_i64, trim) if x_i64 is not None and x_i64.size else np.zeros(0, dtype=np.float32)
    return out_f, out_i


def boundary_tie_columns(x: np.ndarray, trim: int) -> np.ndarray:
    """Columns where the b-th and (b+1)-th smallest distances are equal but the rows at that distance
    hold different values: which of them is kept is the tie rule's choice (here: table order; in the
    reference: an accident of its unstable argsort), and the kept sets may legitimately differ."""
    x = _f32(x)
    k, b = x.shape[0], x.shape[0] - 2 * trim
    if b == k:
        return np.zeros(0, dtype=np.int64)
    key = distance_keys(x)
    srt = np.sort(key, axis=0)
    cand = np.flatnonzero(srt[b - 1] == srt[b])
    out = []
    for j in cand:
        vals = x[key[:, j] == srt[b - 1, j], j]
        if np.unique(vals.view(np.uint32)).size > 1:
            out.append(int(j))
    return np.asarray(out, dtype=np.int64)


def value_bound(x: np.ndarray, trim: int) -> np.ndarray:
    """Per column, the any-order fp32 summation bound over the kept values: 2(b-1) 2^-24 sum|kept| / b."""
    x = _f32(x)
    b = x.shape[0] - 2 * trim
    sabs = np.where(kept_rows(x, trim), np.abs(x.astype(np.float64)), 0.0).sum(axis=0)
    return 2 * (b - 1) * 2.0 ** -24 * sabs / b


def bulyan_theta(k: int, f: int) -> int:
    return min(k - 2 * f, k - 2 - f)


def bulyan_select(dist: np.ndarray, f: int) -> list[int]:
    """The reference's cluster loop, re-sorting every step: NaN sorts last, ties go to the lowest index."""
    k = dist.shape[0]
    remaining, out = list(range(k)), []
    if bulyan_theta(k, f) - 2 * f < 1:
        raise ValueError("too few clients")
    while len(out) < k - 2 * f and len(out) < k - 2 - f:
        m = len(remaining)
        if m - 2 - f < 1:
            raise ValueError("a step sums nothing")
        at = int(np.argsort(ko.scores_of(dist, remaining, f), kind="stable")[0])
        out.append(remaining.pop(at))
    return out


def bulyan(x_f32: np.ndarray, x_i64: np.ndarray, f: int):
    """(selection, fp32 region, int64 region as fp32) of Bulyan on [K, n] rows."""
    sel = bulyan_select(ko.pairwise_sqdist(x_f32, x_i64), f)
    out_f, out_i = nearest_mean(x_f32[sel], x_i64[sel] if x_i64 is not None and x_i64.size else x_i64, f)
    return sel, out_f, out_i
