"""What tests/test_reduction_seams.py (CPU) and tests/test_reduction_seams_gpu.py share: the chunk counts
of plato_agg_pairwise_sqdist and plato_agg_trust_stats as the library itself reports them, the seam of the
chunk rule found from those counts, and the exact inputs.

Chunk rule (csrc/rows.h, chunk_len): a region of n coordinates is cut into chunks of
``unit * max(1, ceil(n / (unit * max_chunks)))`` coordinates.  Up to S = unit * max_chunks coordinates a
chunk is one unit; from S + 1 on it is 2, 3, ... units.  The unit is public (64 * PLATO_AGG_PAIRDIST_CHAIN,
PLATO_AGG_TRUST_TILE), max_chunks is not: S is found as the largest multiple of the unit that still gets
one chunk per unit, from the workspace sizes, which the library computes on the host.
"""

from __future__ import annotations

import functools

import numpy as np

from plato_amd import _lib

DIST, STATS = "dist", "stats"
UNIT = {DIST: 64 * _lib.PLATO_AGG_PAIRDIST_CHAIN, STATS: _lib.PLATO_AGG_TRUST_TILE}


def chunks(kind: str, n: int, k: int = 1) -> int:
    """Chunks of a region of n coordinates: the workspace holds one partial per (chunk, tile, pair slot) for
    the distances and per (chunk, output row) for the statistics."""
    if n == 0:
        return 0  # the library then asks for a token 256 bytes
    if kind == DIST:
        tiles = (k + 31) // 32
        nbytes, per = _lib.lib().plato_agg_pairwise_sqdist_workspace(k, n, 0), tiles * (tiles + 1) // 2 * 1024 * 8
    else:
        nbytes, per = _lib.lib().plato_agg_trust_stats_workspace(k, n, 0), (3 * k + 1) * 8
    assert nbytes > 0 and nbytes % per == 0
    return nbytes // per


@functools.lru_cache(maxsize=None)
def seam(kind: str) -> int:
    """S: the largest n, a multiple of the unit, whose chunks are one unit long."""
    unit = UNIT[kind]
    lo, hi = 1, 1 << 20  # one unit per chunk at lo units, not at hi
    assert chunks(kind, lo * unit) == lo and chunks(kind, hi * unit) < hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if chunks(kind, mid * unit) == mid else (lo, mid)
    return lo * unit


def chunk_len(kind: str, n: int) -> int:
    """Coordinates per chunk of a region of n, restated; checked against the library's count."""
    s = seam(kind)
    clen = UNIT[kind] * max(1, -(-n // s))
    assert chunks(kind, n) == -(-n // clen)
    return clen


def sizes(kind: str) -> dict:
    """The fp32 sizes around the seams: one-unit chunks up to S, two units (the last chunk one coordinate) at
    S + 1, three past 2S, and one two-unit size whose last chunk ends inside a panel or pass."""
    s, unit = seam(kind), UNIT[kind]
    return {"S-1": s - 1, "S": s, "S+1": s + 1, "2S": 2 * s, "2S+1": 2 * s + 1, "ragged": s + 3 * unit + 77}


def _small(rng, shape) -> np.ndarray:
    return rng.integers(-8, 9, shape, dtype=np.int8)


def _apart(rng, row: np.ndarray) -> np.ndarray:
    """A row in [-8, 8] that differs from ``row`` at every coordinate."""
    return ((row.astype(np.int16) + 8 + rng.integers(1, 17, row.shape, dtype=np.int8)) % 17 - 8).astype(np.int8)


def dist_inputs(seed: int, k: int, n_f: int, n_i: int):
    """(x_f32 [K, n_f], x_i64 [K, n_i]) of integers in [-8, 8].  Every odd row differs from the row before it
    at every coordinate, and the last row of an odd K > 1 from row 0: every 8 x 8 block on the diagonal, and
    with it every tile on the diagonal, and the tile of K = 33's last client have a pair whose term is
    non-zero at every coordinate (covered() checks it)."""
    rng = np.random.default_rng(seed)
    both = _small(rng, (k, n_f + n_i))
    for r in range(1, k, 2):
        both[r] = _apart(rng, both[r - 1])
    if k > 1 and k % 2:
        both[k - 1] = _apart(rng, both[0])
    return both[:, :n_f].astype(np.float32), both[:, n_f:].astype(np.int64)


def dist_pairs(k: int):
    """The pairs that dist_inputs keeps apart."""
    return [(r - 1, r) for r in range(1, k, 2)] + ([(0, k - 1)] if k > 1 and k % 2 else [])


def dist_covered(xf: np.ndarray, xi: np.ndarray) -> bool:
    k = xf.shape[0]
    return k == 1 or all(bool((x[i] != x[j]).all()) for x in (xf, xi) for i, j in dist_pairs(k))


def stats_inputs(seed: int, k: int, n_f: int, n_i: int):
    """(x_f32, x_i64, ref [n_f + n_i] float32) of integers in [-8, 8].  The reference vector and the first
    row of every batch of 8 clients are non-zero at every coordinate: |r|^2 and that row's |c|^2 have a
    non-zero term wherever a workgroup of either kind could lose one (stats_covered() checks it)."""
    rng = np.random.default_rng(seed)
    both = _small(rng, (k, n_f + n_i))
    zero = np.zeros((1, n_f + n_i), dtype=np.int8)
    both[::8] = _apart(rng, np.broadcast_to(zero, both[::8].shape))
    ref = _apart(rng, zero[0])
    return both[:, :n_f].astype(np.float32), both[:, n_f:].astype(np.int64), ref.astype(np.float32)


def stats_covered(xf: np.ndarray, xi: np.ndarray, ref: np.ndarray) -> bool:
    return bool((ref != 0).all() and (xf[::8] != 0).all() and (xi[::8] != 0).all())
