"""The CPU half of tests/test_reduction_seams_gpu.py: the chunk counts of plato_agg_pairwise_sqdist and
plato_agg_trust_stats at the seams of the chunk rule (the workspace exports run on the host), and the exact
references (krum_oracle.exact_sqdist, fltrust_oracle.exact_stats) against Python int arithmetic.

The counts are literal on purpose: a change of a kernel's kMaxChunks or of a unit fails here, instead of
silently moving the GPU cases, which derive their sizes from the library, off the seams they are about.
"""

import numpy as np
import pytest

from plato_amd import _lib
from tests import fltrust_oracle as fo
from tests import krum_oracle as ko
from tests import reduction_seams as rs


@pytest.mark.parametrize("kind, unit, s, at_s, past_s, at_2s",
                         [(rs.DIST, 8192, 256 * 8192, 256, 129, 256), (rs.STATS, 1024, 1024 * 1024, 1024, 513, 1024)])
def test_chunk_counts_at_the_seams(kind, unit, s, at_s, past_s, at_2s):
    assert rs.UNIT[kind] == unit and rs.seam(kind) == s
    count = lambda n: rs.chunks(kind, n)  # noqa: E731
    assert [count(n) for n in (1, unit, unit + 1, s - 1, s)] == [1, 1, 2, at_s, at_s]
    assert [count(n) for n in (s + 1, 2 * s, 2 * s + 1)] == [past_s, at_2s, (2 * s) // (3 * unit) + 1]
    assert count(s + 3 * unit + 77) == at_s // 2 + 2
    assert [rs.chunk_len(kind, n) for n in (s, s + 1, 2 * s, 2 * s + 1)] == [unit, 2 * unit, 2 * unit, 3 * unit]
    # the count does not depend on K, and the int64 region follows the same rule with chunks of its own
    for k in (2, 9, 33):
        assert rs.chunks(kind, s + 1, k) == past_s
    if kind == rs.DIST:
        ws = _lib.lib().plato_agg_pairwise_sqdist_workspace
        assert ws(2, s, s) == 2 * at_s * 8192 and ws(2, 5, s + 1) == (1 + past_s) * 8192
    else:
        ws = _lib.lib().plato_agg_trust_stats_workspace
        assert ws(9, s, s) == 2 * at_s * 28 * 8 and ws(9, s, s - 1) == 2 * at_s * 28 * 8
        assert ws(9, 5, s + 1) == (1 + past_s) * 28 * 8


def test_the_sizes_sit_on_the_seams():
    for kind in (rs.DIST, rs.STATS):
        s, unit, sizes = rs.seam(kind), rs.UNIT[kind], rs.sizes(kind)
        assert list(sizes) == ["S-1", "S", "S+1", "2S", "2S+1", "ragged"]
        assert [rs.chunk_len(kind, n) // unit for n in sizes.values()] == [1, 1, 2, 2, 3, 2]
        assert (s + 1) % (2 * unit) == 1                       # the last chunk of S + 1 holds one coordinate
        assert 0 < sizes["ragged"] % (2 * unit) % 128 < 128    # ... of the ragged size ends inside a panel and a pass


def _python_sqdist(xf, xi):
    rows = [[int(v) for v in f] + [int(v) for v in i] for f, i in zip(xf, xi)]
    return [[sum((a - b) ** 2 for a, b in zip(ra, rb)) for rb in rows] for ra in rows]


@pytest.mark.parametrize("k, n_f, n_i", [(1, 7, 0), (2, 300, 5), (3, 257, 0), (9, 130, 3), (33, 0, 40), (33, 40, 1)])
def test_exact_sqdist_equals_python_int_arithmetic(k, n_f, n_i):
    xf, xi = rs.dist_inputs(10 * k + n_i, k, n_f, n_i)
    assert xf.shape == (k, n_f) and xi.shape == (k, n_i) and rs.dist_covered(xf, xi)
    assert max(np.abs(xf).max(initial=0), np.abs(xi).max(initial=0)) <= 8
    want = _python_sqdist(xf, xi)
    for block in (1 << 18, 64, 7):  # one block, several, a ragged last one
        got, largest, term = ko.exact_sqdist(xf, xi, block)
        assert got == want and all(type(v) is int for row in got for v in row)
        assert largest == max(max(row) for row in want) and term <= 256
        assert term >= max((int(a) - int(b)) ** 2 for x in (xf, xi) for col in x.T for a in col for b in col)


def test_exact_sqdist_refuses_what_it_cannot_sum_exactly():
    xf, xi = rs.dist_inputs(1, 2, 9, 2)
    half = xf.copy()
    half[0, 3] = 0.5
    with pytest.raises(AssertionError):
        ko.exact_sqdist(half, xi)
    big = xi.copy()
    big[1, 0] = (1 << 24) + 1  # not a float32
    with pytest.raises(AssertionError):
        ko.exact_sqdist(xf, big)


def test_inputs_are_kept_apart_where_they_say():
    xf, xi = rs.dist_inputs(5, 9, 500, 7)
    assert rs.dist_pairs(9) == [(0, 1), (2, 3), (4, 5), (6, 7), (0, 8)] and rs.dist_pairs(2) == [(0, 1)]
    assert rs.dist_covered(xf, xi)
    xf[3, 77] = xf[2, 77]
    assert not rs.dist_covered(xf, xi)
    xf, xi, ref = rs.stats_inputs(5, 9, 500, 7)
    assert rs.stats_covered(xf, xi, ref) and (xf[1:8] == 0).any()
    assert np.abs(ref).max() <= 8 and np.abs(xf).max() <= 8 and np.abs(xi).max() <= 8
    ref[499] = 0
    assert not rs.stats_covered(xf, xi, ref)


def _python_stats(xf, xi, ref, eps):
    rows = [[int(v) for v in f] + [int(v) for v in i] for f, i in zip(xf, xi)]
    r = [int(v) for v in ref]
    e = int(eps)
    sums = [sum(c * v for c, v in zip(row, r)) for row in rows]
    sums += [sum(c * c for c in row) for row in rows]
    sums += [sum((c + e) ** 2 for c in row) for row in rows]
    mags = [sum(abs(c * v) for c, v in zip(row, r)) for row in rows] + sums[len(rows):]
    return sums + [sum(v * v for v in r)], max(mags + [sum(v * v for v in r)])


@pytest.mark.parametrize("eps", [0.0, 1.0])
@pytest.mark.parametrize("k, n_f, n_i", [(1, 300, 5), (8, 257, 0), (9, 130, 3), (3, 0, 40)])
def test_exact_stats_equals_python_int_arithmetic(k, n_f, n_i, eps):
    xf, xi, ref = rs.stats_inputs(20 * k + n_i, k, n_f, n_i)
    assert rs.stats_covered(xf, xi, ref) and ref.shape == (n_f + n_i,)
    got, mag = fo.exact_stats(xf, xi, ref, np.float32(eps))
    want, want_mag = _python_stats(xf, xi, ref, eps)
    assert got == want and mag == want_mag and all(type(v) is int for v in got)
    assert (got[2 * k:3 * k] == got[k:2 * k]) == (eps == 0)
    # against the module's general restatement, which is exact at these sizes too
    exp, _ = fo.stats(fo.columns(xf, xi), ref, np.float32(eps))
    assert exp.tolist() == [float(v) for v in got]
