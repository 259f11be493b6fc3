"""CPU restatements of plato_agg_trust_stats and plato_agg_scaled_sum (include/plato_agg.h) and of the
whole Fl-trust pipeline (examples/detector/aggregations.py:403-453 of the reference): numpy, with the
scalars of ``plato_amd.trust``.

``x_f32``: [K, n] float32; ``x_i64``: [K, m] int64, promoted to float32 with round to nearest even, as
``flatten_weights``' torch.cat does.  The statistics are exact sums (``math.fsum`` over the float64
products, which are exact for fp32 operands) where the sizes allow it, plain float64 sums otherwise.
"""

from __future__ import annotations

import math

import numpy as np

from tests.krum_oracle import columns, mean_rows  # noqa: F401

EPS32 = np.float32(1e-9)


def mean(x_f32: np.ndarray, x_i64: np.ndarray) -> np.ndarray:
    """The sequential fp32 mean of the rows in table order, both regions, as one [n + m] vector."""
    mf, mi = mean_rows(x_f32, x_i64, range(x_f32.shape[0]))
    return np.concatenate([mf, mi])


def _sum(terms: np.ndarray, exact: bool) -> float:
    if exact:
        try:
            return math.fsum(terms.tolist())
        except (OverflowError, ValueError):  # inf / NaN among the terms: IEEE addition decides
            pass
    with np.errstate(invalid="ignore", over="ignore"):
        return float(np.sum(terms))


def stats(cols: np.ndarray, ref: np.ndarray, eps=EPS32, exact: bool = True):
    """(values [3K + 1] float64, sum|terms| [3K + 1] float64) of plato_agg_trust_stats over the promoted
    columns ``cols`` [K, D] and the reference vector ``ref`` [D] (both float32)."""
    k = cols.shape[0]
    c = cols.astype(np.float64)
    r = ref.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        ce = (cols + np.float32(eps)).astype(np.float32).astype(np.float64)  # one fp32 addition
        out, mag = np.empty(3 * k + 1), np.empty(3 * k + 1)
        for i in range(k):
            for at, terms in ((i, c[i] * r), (k + i, c[i] * c[i]), (2 * k + i, ce[i] * ce[i])):
                out[at], mag[at] = _sum(terms, exact), float(np.sum(np.abs(terms)))
        out[3 * k], mag[3 * k] = _sum(r * r, exact), float(np.sum(r * r))
    return out, mag


def exact_stats(x_f32: np.ndarray, x_i64: np.ndarray, ref: np.ndarray, eps):
    """(sums, largest sum of |terms|) of plato_agg_trust_stats on rows, a reference vector and an eps that
    all hold small integers: the 3K + 1 sums as Python ints, formed in int64 (the bound on the inputs, asserted,
    keeps every sum below 2^62).  No partial sum of any order exceeds its row's sum of |terms|."""
    assert x_f32.dtype == np.float32 and x_i64.dtype == np.int64 and ref.dtype == np.float32
    n_f, k = x_f32.shape[1], x_f32.shape[0]
    e = int(eps)
    assert e == eps and ref.shape == (n_f + x_i64.shape[1],)
    out, mag = [0] * (3 * k + 1), [0] * (3 * k + 1)
    for x, r32 in ((x_f32, ref[:n_f]), (x_i64, ref[n_f:])):
        c, r = x.astype(np.int64), r32.astype(np.int64)
        assert np.array_equal(c.astype(np.float32), x) and np.array_equal(r.astype(np.float32), r32)  # fp32 holds them
        top = max(int(np.abs(c).max(initial=0)) + abs(e), int(np.abs(r).max(initial=0)))
        assert c.shape[1] * top * top < 2 ** 62
        for i in range(k):
            for at, terms in ((i, c[i] * r), (k + i, c[i] * c[i]), (2 * k + i, (c[i] + e) * (c[i] + e))):
                out[at] += int(terms.sum())
                mag[at] += int(np.abs(terms).sum())
        out[3 * k] += int((r * r).sum())
        mag[3 * k] += int((r * r).sum())
    return out, max(mag)


def scaled_sum(cols: np.ndarray, mul, div, post) -> np.ndarray:
    """plato_agg_scaled_sum: per coordinate the sequential fp32 sum over the rows of
    fp32(fp32(fp32(c * mul_k) / div_k) * post)."""
    mul, div, post = np.asarray(mul, dtype=np.float32), np.asarray(div, dtype=np.float32), np.float32(post)
    acc = np.zeros(cols.shape[1], dtype=np.float32)
    with np.errstate(all="ignore"):
        for k in range(cols.shape[0]):
            t = (cols[k] * mul[k]).astype(np.float32)
            t = (t / div[k]).astype(np.float32)
            t = (t * post).astype(np.float32)
            acc = (acc + t).astype(np.float32)
    return acc


def fltrust(x_f32: np.ndarray, x_i64: np.ndarray, device_stats=None, exact: bool = False):
    """(output [D] float32, scalars) of the whole pipeline: sequential mean, statistics (``device_stats``
    if given, else this module's), ``plato_amd.trust.fltrust_weights``, sequential scaled sum."""
    from plato_amd.trust import fltrust_weights

    cols = columns(x_f32, x_i64)
    k = cols.shape[0]
    st = stats(cols, mean(x_f32, x_i64), exact=exact)[0] if device_stats is None else np.asarray(device_stats)
    scal = fltrust_weights(st, k)
    return scaled_sum(cols, scal["weights"], scal["div"], scal["nm"]), scal


def gains(scal) -> np.ndarray:
    """g_k = w_k / div_k * nm in float64 from a side's fp32 scalars."""
    with np.errstate(all="ignore"):
        return (np.asarray(scal["weights"], dtype=np.float64) / np.asarray(scal["div"], dtype=np.float64)
                * float(scal["nm"]))


def output_bound(cols: np.ndarray, g: np.ndarray, g_ref: np.ndarray) -> np.ndarray:
    """Per coordinate: sum_k |c_k[e]| * (|g_k - g_k^ref| + (2K + 4) * 2^-24 * max(|g_k|, |g_k^ref|)) + 3K * 2^-149
    (three roundings per term and any-order fp32 summation on both sides)."""
    k = cols.shape[0]
    per = np.abs(g - g_ref) + (2 * k + 4) * 2.0 ** -24 * np.maximum(np.abs(g), np.abs(g_ref))
    return np.abs(cols.astype(np.float64)).T @ per + 3 * k * 2.0 ** -149


def cosine64(cols: np.ndarray, m: np.ndarray) -> np.ndarray:
    """The reference's cosine formula in float64 on a given mean vector."""
    c, m = cols.astype(np.float64), m.astype(np.float64)
    nm = math.sqrt(float(m @ m))
    return np.array([float(c[i] @ m) / (nm + 1e-9) / (math.sqrt(float(c[i] @ c[i])) + 1e-9) for i in range(c.shape[0])])
