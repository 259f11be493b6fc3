"""CPU restatements of plato_agg_pairwise_sqdist, plato_agg_mean_rows (include/plato_agg.h) and of the
reference's Multi-Krum selection (examples/detector/aggregations.py:176-216): numpy only.

``x_f32``: [K, n] float32; ``x_i64``: [K, m] int64, promoted to float32 with round to nearest even, as
``flatten_weights``' torch.cat does.  The distances are fp32 differences, squared and summed in float64
(the kernel's fp32 chains are within (PLATO_AGG_PAIRDIST_CHAIN + 1) * 2^-24 of it).  The selection
re-sorts every step, as the reference does: the product's incremental one (plato_amd.krum) is checked
against it.
"""

from __future__ import annotations

import numpy as np


def columns(x_f32: np.ndarray, x_i64: np.ndarray) -> np.ndarray:
    """[K, n + m] float32: the flattened rows, fp32 region first, counters promoted."""
    parts = [np.ascontiguousarray(x_f32, dtype=np.float32)]
    if x_i64 is not None and x_i64.size:
        assert x_i64.dtype == np.int64
        parts.append(x_i64.astype(np.float32))  # RNE
    return np.concatenate(parts, axis=1)


def pairwise_sqdist(x_f32: np.ndarray, x_i64: np.ndarray) -> np.ndarray:
    """[K, K] float64: sum of the squared fp32 differences; the diagonal is +0 whatever the row holds."""
    c = columns(x_f32, x_i64)
    k = c.shape[0]
    out = np.zeros((k, k), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for lo in range(0, c.shape[1], 1 << 20):  # column blocks: bounded temporaries at full model size
            blk = c[:, lo:lo + (1 << 20)]
            for i in range(k):
                d = (blk - blk[i]).astype(np.float64)  # the fp32 difference, widened
                out[i] += (d * d).sum(axis=1)
    out[np.arange(k), np.arange(k)] = 0.0
    return out


def exact_sqdist(x_f32: np.ndarray, x_i64: np.ndarray, block: int = 1 << 18):
    """(sums, largest sum, largest term) of the squared distances of rows that hold small integers: the
    sums as [K][K] Python ints, exact.  They come from a float64 Gram product in column blocks,
    |c_i - c_j|^2 = G_ii + G_jj - 2 G_ij: every product and every partial of a block is an integer below
    block * max|c|^2 < 2^53 (asserted), so a block's G is exact in whatever order the product adds, and the
    blocks are added as int64.  Every term of a distance is >= 0, so the largest partial sum that any order of
    any pair can form is the largest sum; the largest term is bounded by (max c - min c)^2."""
    assert x_f32.dtype == np.float32 and x_i64.dtype == np.int64 and x_f32.shape[0] == x_i64.shape[0]
    k = x_f32.shape[0]
    gram = np.zeros((k, k), dtype=np.int64)
    lo, hi = 0, 0
    for x in (x_f32, x_i64):
        for at in range(0, x.shape[1], block):
            c = x[:, at:at + block].astype(np.float64)
            assert np.array_equal(c, np.rint(c)) and np.array_equal(c.astype(np.float32), c)  # integers that fp32 holds
            top = float(np.abs(c).max())
            assert c.shape[1] * top * top < 2.0 ** 53
            g = c @ c.T
            assert np.array_equal(g, np.rint(g))
            gram += g.astype(np.int64)
            lo, hi = min(lo, int(c.min())), max(hi, int(c.max()))
    diag = np.diagonal(gram)
    assert int(diag.max(initial=0)) < 2 ** 60  # the int64 combination below does not wrap
    dist = diag[:, None] + diag[None, :] - 2 * gram
    assert (dist >= 0).all() and not np.diagonal(dist).any()
    return dist.tolist(), int(dist.max()), (hi - lo) ** 2


def select(dist: np.ndarray, f: int = 2) -> list[int]:
    """Multi-Krum's selection order: NaN sorts last, ties go to the lowest client index."""
    remaining = list(range(dist.shape[0]))
    if len(remaining) <= 2 * f + 2:
        raise ValueError("too few clients")
    out = []
    while len(remaining) > 2 * f + 2:
        m = len(remaining)
        sub = np.sort(dist[np.ix_(remaining, remaining)], axis=1)  # NaN last
        with np.errstate(invalid="ignore"):
            scores = sub[:, : m - 2 - f].sum(axis=1)
        at = int(np.argsort(scores, kind="stable")[0])
        out.append(remaining.pop(at))
    return out


def scores_of(dist: np.ndarray, remaining, f: int = 2) -> np.ndarray:
    """The scores of one selection step over ``remaining``."""
    m = len(remaining)
    sub = np.sort(dist[np.ix_(remaining, remaining)], axis=1)
    return sub[:, : m - 2 - f].sum(axis=1)


def mean_rows(x_f32: np.ndarray, x_i64: np.ndarray, order):
    """(fp32 region, int64 region as fp32): the sequential fp32 row sum in ``order``, divided by fp32(m)."""
    def one(x):
        acc = np.zeros(x.shape[1], dtype=np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            for r in order:
                acc = (acc + x[r].astype(np.float32)).astype(np.float32)
            return (acc / np.float32(len(order))).astype(np.float32)
    out_f = one(x_f32) if x_f32.size else np.zeros(0, dtype=np.float32)
    out_i = one(x_i64) if x_i64 is not None and x_i64.size else np.zeros(0, dtype=np.float32)
    return out_f, out_i


def mean_bound(x_f32_or_cols: np.ndarray, order, ref: np.ndarray) -> np.ndarray:
    """Per coordinate, the bound on |sequential mean - any-order fp32 mean| of rows ``order``:
    2(m-1) * 2^-24 * sum_k|x_k| / m  +  2 * 2^-24 * |ref|  +  2^-149
    (the any-order summation bound applied to both sides, plus the two divisions)."""
    m = len(order)
    u = 2.0 ** -24
    sabs = np.abs(x_f32_or_cols[list(order)].astype(np.float64)).sum(axis=0)
    return 2 * (m - 1) * u * sabs / m + 2 * u * np.abs(ref.astype(np.float64)) + 2.0 ** -149
