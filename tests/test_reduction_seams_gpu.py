"""plato_agg_pairwise_sqdist (csrc/krum.hip) and plato_agg_trust_stats (csrc/trust.hip) where a coordinate
chunk takes several chains or passes, pinned with no tolerance at all.

Chunk rule (csrc/rows.h): a region of n coordinates is cut into chunks of unit * max(1, ceil(n / S))
coordinates, S = unit * max_chunks, one workgroup per chunk (and tile, or client batch).  The unit is one
fp32 chain, 64 * PLATO_AGG_PAIRDIST_CHAIN = 8,192 coordinates, for the distances (S = 256 units = 2,097,152)
and PLATO_AGG_TRUST_TILE = 1,024 for the statistics (S = 1,024 units = 1,048,576).  Up to S a workgroup ends
with its first chain, or after two passes of 512; past S it flushes a full chain in the middle of its chunk
((p + 1) % kChainPanels == 0) and goes round the pass loop again, the last chunk may hold one coordinate, and
the finish kernels add up to 256 + 256 and 1,024 + 1,024 partials (fp32 and int64 region), the latter exactly
the size of trust_final_kernel's LDS array.  Every real model is past S; the other direct tests stop at three
one-unit chunks, and at full size a lost coordinate is 1e-7 of a distance, far inside their tolerance.

Sizes: S - 1, S, S + 1 (two-unit chunks, the last one a single coordinate), 2S, 2S + 1 (three units) and
S + 3 units + 77 (two units, the last chunk ends inside a panel and a pass); S comes from the library's own
workspace sizes (tests/reduction_seams.py), and tests/test_reduction_seams.py pins the counts on the CPU.

Exact inputs: rows, reference vector and counters are integers in [-8, 8].  d = c_i - c_j is exact in fp32, a
chain of 128 fma(d, d, acc) stays below 128 * 256 < 2^24 and is exact, every float64 partial is an integer
below n * 256 < 2^53; c * r, c * c and (c + eps)^2 with eps in {0, 1} likewise.  So the device must EQUAL the
integer sums of the host (krum_oracle.exact_sqdist, fltrust_oracle.exact_stats) in whatever order it adds:
a coordinate dropped or counted twice at a chunk, chain or pass seam, or a partial the finish kernel misses,
fails.  The bounds are asserted from the inputs.  A lost coordinate whose term is zero would not show, so the
inputs keep a pair of rows apart, and the reference vector and a row of every batch non-zero, at every
coordinate (checked here); a lost and a doubled coordinate could cancel, so every size runs with two seeds.
A second test moves a single 1 through all-zero rows on the device and so names the coordinate that is lost.
The guards of device_sqdist / device_stats behind output and workspace hold at these workspace sizes too.
"""

import numpy as np
import pytest
import torch

from plato_amd import _lib
from tests import fltrust_oracle as fo
from tests import krum_oracle as ko
from tests import reduction_seams as rs
from tests import test_fltrust_gpu as tg
from tests import test_krum_gpu as kg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CHAIN = _lib.PLATO_AGG_PAIRDIST_CHAIN
NAMES = ("S-1", "S", "S+1", "2S", "2S+1", "ragged")
SEEDS = (0, 1)
bits = kg.bits


def floats(ints):
    """The integers as float64, nested as given: exact below 2^53, which the callers assert first."""
    return np.array(ints, dtype=np.float64).tolist()


# ------------------------------------------------------------------ exact sums
def check_sqdist(seed, k, n_f, n_i, order=None):
    xf, xi = rs.dist_inputs(seed, k, n_f, n_i)
    assert rs.dist_covered(xf, xi)
    want, largest, term = ko.exact_sqdist(xf, xi)
    assert largest < 2 ** 53 and CHAIN * term < 2 ** 24  # from the inputs: every partial of the device is exact
    got = kg.device_sqdist(xf, xi, order)
    if order is not None:
        want = [[want[i][j] for j in order] for i in order]
    assert got.tolist() == floats(want), (seed, k, n_f, n_i)
    assert not bits(np.diagonal(got)).any()
    return xf, xi, got


def check_stats(seed, k, n_f, n_i, eps):
    xf, xi, ref = rs.stats_inputs(seed, k, n_f, n_i)
    assert rs.stats_covered(xf, xi, ref)
    want, mag = fo.exact_stats(xf, xi, ref, eps)
    assert mag < 2 ** 53
    got = tg.device_stats(xf, xi, ref, eps=np.float32(eps))
    assert got.tolist() == floats(want), (seed, k, n_f, n_i, eps)
    if eps == 0:
        assert np.array_equal(bits(got[2 * k:3 * k]), bits(got[k:2 * k]))
    return xf, xi, ref, got


@pytest.mark.parametrize("k", (2, 3))
@pytest.mark.parametrize("name", NAMES)
def test_distances_equal_the_integer_sums_at_the_seams(name, k):
    n_f = rs.sizes(rs.DIST)[name]
    for seed in SEEDS:
        check_sqdist(1000 * k + seed, k, n_f, (0, 5)[seed])


def test_distances_of_three_tiles_past_the_seam():
    check_sqdist(33, 33, rs.seam(rs.DIST) + 1, 5)


@pytest.mark.parametrize("seed", SEEDS)
def test_distances_with_counters_past_the_seam(seed):
    check_sqdist(40 + seed, 2, 5, rs.seam(rs.DIST) + 1)


@pytest.mark.parametrize("seed", SEEDS)
def test_distances_with_the_most_chunks_in_both_regions(seed):
    s = rs.seam(rs.DIST)
    assert rs.chunks(rs.DIST, s) == rs.chunks(rs.DIST, 2 * s)  # no size has more
    check_sqdist(50 + seed, 2, s, s)


@pytest.mark.parametrize("k", (1, 8, 9))
@pytest.mark.parametrize("name", NAMES)
def test_statistics_equal_the_integer_sums_at_the_seams(name, k):
    n_f = rs.sizes(rs.STATS)[name]
    for seed in SEEDS:
        check_stats(2000 * k + seed, k, n_f, (0, 5)[seed], (0.0, 1.0)[seed])
    if name == "S+1":  # eps = 0 next to counters, once
        check_stats(2000 * k + 2, k, n_f, 5, 0.0)


@pytest.mark.parametrize("k", (1, 9))
def test_statistics_with_counters_past_the_seam(k):
    for seed in SEEDS:
        check_stats(60 + 10 * k + seed, k, 5, rs.seam(rs.STATS) + 1, (0.0, 1.0)[seed])


@pytest.mark.parametrize("short", (0, 1))
def test_statistics_with_partials_that_fill_the_finish_kernels_array(short):
    """n_f32 = n_i64 = S: 1,024 + 1,024 partials per output row, all of part[]; and its neighbour."""
    s = rs.seam(rs.STATS)
    assert rs.chunks(rs.STATS, s) == rs.chunks(rs.STATS, 2 * s)  # no size has more
    for seed in SEEDS:
        check_stats(80 + seed, 9, s, s - short, (0.0, 1.0)[seed])


# ------------------------------------------------------------------ one coordinate at a time
def positions(kind, n):
    """The first and the last coordinate, both sides of the first and of the last chunk seam, both sides of
    the first chain (or pass-loop trip) boundary inside a chunk."""
    clen, last = rs.chunk_len(kind, n), rs.chunks(kind, n) - 1
    assert clen == 2 * rs.UNIT[kind] and last >= 2 and last * clen < n
    at = [0, n - 1, clen - 1, clen, last * clen - 1, last * clen, clen // 2 - 1, clen // 2]
    return sorted(set(at))


def zero_rows(n_f, n_i):
    df = torch.zeros((2, n_f), dtype=torch.float32, device=DEV)
    di = torch.zeros((2, n_i), dtype=torch.int64, device=DEV)
    tf = torch.tensor([df.data_ptr(), df.data_ptr() + 4 * n_f], dtype=torch.int64, device=DEV)
    ti = torch.tensor([di.data_ptr(), di.data_ptr() + 8 * n_i], dtype=torch.int64, device=DEV)
    return df, di, tf, ti


@pytest.mark.parametrize("name", ("S+1", "ragged"))
def test_every_single_coordinate_reaches_its_distance(name):
    n_f, n_i = rs.sizes(rs.DIST)[name], 5
    df, di, tf, ti = zero_rows(n_f, n_i)
    assert not bits(kg.launch_sqdist(tf, ti, n_f, n_i)).any()  # all rows zero: all +0
    for row, at in [(df, p) for p in positions(rs.DIST, n_f)] + [(di, 2)]:
        row[1, at] = 1
        got = kg.launch_sqdist(tf, ti, n_f, n_i)
        row[1, at] = 0
        assert got.tolist() == [[0.0, 1.0], [1.0, 0.0]], (name, "i64" if row is di else "f32", at)
        assert not bits(np.diagonal(got)).any()


@pytest.mark.parametrize("name", ("S+1", "ragged"))
def test_every_single_coordinate_reaches_its_statistics(name):
    n_f, n_i = rs.sizes(rs.STATS)[name], 5
    df, di, tf, ti = zero_rows(n_f, n_i)
    rf, ri = torch.ones(n_f, device=DEV), torch.ones(n_i, device=DEV)
    zero = tg.launch_stats(tf, ti, rf, ri, 0.0, n_f, n_i)
    assert not bits(zero[:6]).any() and zero[6] == n_f + n_i
    for row, at in [(df, p) for p in positions(rs.STATS, n_f)] + [(di, 2)]:
        row[1, at] = 1
        got = tg.launch_stats(tf, ti, rf, ri, 0.0, n_f, n_i)
        row[1, at] = 0
        where = (name, "i64" if row is di else "f32", at)
        assert got[[1, 3, 5]].tolist() == [1.0, 1.0, 1.0], where  # row 1: dot, |c|^2, |c + 0|^2
        assert not bits(got[[0, 2, 4]]).any(), where              # row 0: +0
        assert got[6] == n_f + n_i, where                         # |r|^2


# ------------------------------------------------------------------ order and K past the seam
def test_distances_past_the_seam_do_not_depend_on_order_or_k():
    k, n_f, n_i = 9, rs.seam(rs.DIST) + 1 + 77, 3
    xf, xi, first = check_sqdist(9, k, n_f, n_i)
    assert np.array_equal(bits(first), bits(kg.device_sqdist(xf, xi)))  # two runs
    perm = np.random.default_rng(9).permutation(k)
    assert perm.tolist() != list(range(k))
    assert np.array_equal(bits(kg.device_sqdist(xf, xi, perm)), bits(first[np.ix_(perm, perm)]))
    sub = [8, 3, 0, 5]  # K = 4: one block, the same pairs
    assert np.array_equal(bits(kg.device_sqdist(xf, xi, sub)), bits(first[np.ix_(sub, sub)]))


def test_statistics_past_the_seam_do_not_depend_on_order_or_k():
    k, n_f, n_i = 9, rs.seam(rs.STATS) + 1 + 77, 5
    xf, xi, ref, first = check_stats(9, k, n_f, n_i, 1.0)
    again = lambda order: tg.device_stats(xf, xi, ref, eps=np.float32(1.0), order=order)  # noqa: E731
    assert np.array_equal(bits(first), bits(again(None)))  # two runs
    perm = np.random.default_rng(9).permutation(k)
    assert perm.tolist() != list(range(k))
    moved = again(perm)
    for part in range(3):
        assert np.array_equal(bits(moved[part * k:(part + 1) * k]), bits(first[part * k:(part + 1) * k][perm]))
    sub = [8, 3, 0]  # K = 3: one batch; client 8 leaves the batch it had to itself
    small = again(sub)
    for part in range(3):
        assert np.array_equal(bits(small[part * 3:part * 3 + 3]), bits(first[part * k:(part + 1) * k][sub]))
    assert bits(moved[-1:]) == bits(small[-1:]) == bits(first[-1:])


# ------------------------------------------------------------------ the small grid, exactly
@pytest.mark.parametrize("k", kg.KS_SMALL + kg.KS_LARGE)
def test_distances_of_every_client_count_equal_the_integer_sums(k):
    check_sqdist(300 + k, k, rs.UNIT[rs.DIST] + 1, 3)


@pytest.mark.parametrize("k", tg.KS_SMALL + tg.KS_LARGE)
def test_statistics_of_every_client_count_equal_the_integer_sums(k):
    check_stats(400 + k, k, rs.UNIT[rs.STATS] + 1, 5, 1.0)
    check_stats(400 + k, k, rs.UNIT[rs.STATS] + 1, 5, 0.0)
