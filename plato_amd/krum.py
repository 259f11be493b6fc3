"""Multi-Krum's and Bulyan's selections on the host: numpy over the float64 distance matrix of the device.

Restates the loop of ``aggregations.multi_krum`` (the reference's examples/detector/aggregations.py:
176-216) on the K x K matrix of squared distances that ``plato_agg_pairwise_sqdist`` computes once,
where the reference recomputes the distances of the remaining clients at every step:

    remaining = all clients, in order
    while len(remaining) > 2f + 2:
        m = len(remaining)
        score_i = sum of the m - 2 - f smallest distances from i to the remaining clients
                  (its own 0 included; NaN sorts last, as torch.sort does)
        pick the smallest score (NaN scores rank last, as torch.argsort does), append it to the
        result, remove it from remaining

Ties between scores go to the lowest client index.  The reference's ``torch.argsort`` is not stable,
so which of two equal scores it takes is an accident: this is a documented divergence.  ``K <= 2f + 2``
raises ``ValueError``: the reference selects nothing there and fails in ``torch.mean`` of an empty list.

``bulyan_select`` is the same step run min(K - 2f, K - 2 - f) times (aggregations.py:86-123).

Every row is sorted once; when a client leaves, its entry is deleted from every remaining row, so a
step costs one pass over the m x m table instead of m sorts.
"""

from __future__ import annotations

import numpy as np


def multi_krum_select(dist: np.ndarray, f: int = 2) -> list[int]:
    """Client indices in Multi-Krum's selection order (``K - 2f - 2`` of them)."""
    dist = _square(dist)
    f = int(f)
    if f < 0:
        raise ValueError("f must be >= 0")
    k = dist.shape[0]
    if k <= 2 * f + 2:
        raise ValueError(f"Multi-Krum with f = {f} needs more than {2 * f + 2} clients, got {k}")
    return _select(dist, f, k - 2 * f - 2)


def bulyan_select(dist: np.ndarray, f: int) -> list[int]:
    """Client indices of Bulyan's cluster in selection order: ``min(K - 2f, K - 2 - f)`` of them.

    The loop of ``aggregations.bulyan`` (aggregations.py:86-123): Multi-Krum's step, repeated until
    the cluster holds theta = min(K - 2f, K - 2 - f) clients, where K is the number of rows of
    ``dist`` (the reference reads ``clients.total_clients``; the two agree whenever every client
    reports).  ``ValueError`` when theta - 2f < 1 (the coordinate-wise step after the selection would
    average nothing) or when a step would sum no distance at all (m - 2 - f < 1).  For f <= 2 the last
    steps sum one term, the exact +0 of the diagonal: every score ties and the lowest remaining index
    is picked.
    """
    dist = _square(dist)
    f = int(f)
    if f < 0:
        raise ValueError("f must be >= 0")
    k = dist.shape[0]
    theta = min(k - 2 * f, k - 2 - f)
    if theta - 2 * f < 1 or k - theta + 1 - 2 - f < 1:
        raise ValueError(f"Bulyan with f = {f} needs at least {bulyan_min_clients(f)} clients, got {k}")
    return _select(dist, f, theta)


def bulyan_min_clients(f: int) -> int:
    """The smallest K at which Bulyan's cluster keeps a value: theta - 2f >= 1 for both forms of theta."""
    return max(4 * int(f) + 1, 3 * int(f) + 3)


def _square(dist) -> np.ndarray:
    dist = np.asarray(dist, dtype=np.float64)
    if dist.ndim != 2 or dist.shape[0] != dist.shape[1]:
        raise ValueError(f"distance matrix must be square, got shape {dist.shape}")
    return dist


def _select(dist: np.ndarray, f: int, steps: int) -> list[int]:
    """``steps`` selection steps over the sorted-rows table: at each, the client with the smallest sum
    of its m - 2 - f smallest distances to the m remaining clients leaves for the result."""
    remaining = np.arange(dist.shape[0])
    # per remaining client (row): the remaining clients in ascending distance (stable; NaN last) and
    # those distances
    by_dist = np.argsort(dist, axis=1, kind="stable")
    sorted_d = np.take_along_axis(dist, by_dist, axis=1)
    selected: list[int] = []
    for _ in range(steps):
        m = remaining.size
        if m - 2 - f < 1:
            raise ValueError(f"a selection step over {m} clients with f = {f} sums no distance")
        with np.errstate(invalid="ignore"):  # inf + -inf cannot occur (distances are >= 0 or NaN); NaN may
            scores = sorted_d[:, : m - 2 - f].sum(axis=1)
        at = int(np.argsort(scores, kind="stable")[0])  # NaN last; rows are in client order: lowest index wins
        pick = int(remaining[at])
        selected.append(pick)
        keep_rows = np.arange(m) != at
        keep = by_dist[keep_rows] != pick  # exactly one entry per row
        by_dist = by_dist[keep_rows][keep].reshape(m - 1, m - 1)
        sorted_d = sorted_d[keep_rows][keep].reshape(m - 1, m - 1)
        remaining = remaining[keep_rows]
    return selected
