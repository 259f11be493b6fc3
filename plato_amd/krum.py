"""Multi-Krum's selection on the host: numpy over the float64 distance matrix of the device.

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

Every row is sorted once; when a client leaves, its entry is deleted from every remaining row, so a
step costs one pass over the m x m table instead of m sorts.
"""

from __future__ import annotations

import numpy as np


def multi_krum_select(dist: np.ndarray, f: int = 2) -> list[int]:
    """Client indices in Multi-Krum's selection order (``K - 2f - 2`` of them)."""
    dist = np.asarray(dist, dtype=np.float64)
    if dist.ndim != 2 or dist.shape[0] != dist.shape[1]:
        raise ValueError(f"distance matrix must be square, got shape {dist.shape}")
    f = int(f)
    if f < 0:
        raise ValueError("f must be >= 0")
    k = dist.shape[0]
    if k <= 2 * f + 2:
        raise ValueError(f"Multi-Krum with f = {f} needs more than {2 * f + 2} clients, got {k}")
    remaining = np.arange(k)
    # per remaining client (row): the remaining clients in ascending distance (stable; NaN last) and
    # those distances
    by_dist = np.argsort(dist, axis=1, kind="stable")
    sorted_d = np.take_along_axis(dist, by_dist, axis=1)
    selected: list[int] = []
    while remaining.size > 2 * f + 2:
        m = remaining.size
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
