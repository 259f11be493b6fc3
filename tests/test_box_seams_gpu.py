"""The two box kernels at their seams: direct calls of plato_agg_submodel_mean and plato_agg_elastic_mean on
the tables of tests/box_seams.py, every result compared bit for bit with its numpy restatement over the whole
output region (sentinel-filled, guard elements behind it, guard bytes behind the table workspace).

What the sections walk around (plato_amd/csrc/boxes.h, submodel.hip, elastic.hip): a workgroup of 256 lanes
finds its entry by a binary search of the entries' first tiles and owns one tile of 1,024 consecutive elements,
a lane four of them 256 apart; a box whose leading extent ends at or before the tile's first row is skipped on
scalar values, one that covers no lane of a wave by a ballot; the elastic kernel is compiled per number of view
dims from the first that is not 1; and entries of 2^30 elements and more are indexed in 64 bits.  Values are
seeded normals: special values are pinned in tests/test_submodel_gpu.py and tests/test_elastic_gpu.py.

The two wide tests need about 13 GB of device memory each (one after the other); measured on an MI355X, see
DESIGN.md §22.
"""

from math import prod

import numpy as np
import pytest
import torch

from plato_amd import _lib
from tests import box_seams as bs
from tests.test_box_seams import SEARCH_SIZES, layouts_of

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD = 64
PAD = 0x5A
SENTINEL = float(bs.SENTINEL)


def mean(kind, d_g, table, k, row_len, entries, boxes, work, out, n_out):
    stream = torch.cuda.current_stream(DEV).cuda_stream
    if kind == "submodel":
        _lib.call("plato_agg_submodel_mean", d_g.data_ptr(), table.data_ptr(), k, row_len.ctypes.data,
                  entries.ctypes.data, boxes.ctypes.data, len(entries), work.data_ptr(), out.data_ptr(), n_out, stream)
    else:
        _lib.call("plato_agg_elastic_mean", d_g.data_ptr(), table.data_ptr(), k, row_len.ctypes.data,
                  entries.ctypes.data, len(entries), boxes.ctypes.data, len(boxes), work.data_ptr(), out.data_ptr(),
                  n_out, stream)
    torch.cuda.synchronize()


def workspace(kind, k, n_entries, n_boxes):
    nbytes = (_lib.lib().plato_agg_submodel_tables_bytes(k, n_entries) if kind == "submodel"
              else _lib.lib().plato_agg_elastic_tables_bytes(n_entries, n_boxes))
    assert nbytes
    return nbytes, torch.full((nbytes + 256,), PAD, dtype=torch.uint8, device=DEV)


def on_device(t: bs.Tables) -> np.ndarray:
    """The output region after one call; the guards behind it and behind the workspace are checked here."""
    flat, starts = bs.pack_rows(t.rows)
    d_flat = torch.from_numpy(flat).to(DEV)
    table = torch.from_numpy(np.array([d_flat.data_ptr() + 4 * s for s in starts], dtype=np.int64)).to(DEV)
    d_g = torch.from_numpy(t.gflat).to(DEV)
    out = torch.full((t.n_out + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    nbytes, work = workspace(t.kind, t.k, len(t.entries), len(t.boxes))
    mean(t.kind, d_g, table, t.k, t.row_len, t.entries, t.boxes, work, out, t.n_out)
    got = out.cpu().numpy()
    assert (got[t.n_out:] == bs.SENTINEL).all() and bool((work[nbytes:] == PAD).all())
    return got[:t.n_out]


def check(t: bs.Tables, what=""):
    """The device's output region equals the restatement's bit for bit; returns the counts."""
    want, counts = bs.restate(t)
    got = on_device(t)
    if got.tobytes() != want.tobytes():
        e, f = bs.first_difference(t, got, want)
        where = f"entry {e} {t.views[e]}, flat index {f}" if e is not None else f"outside the entries, element {f}"
        raise AssertionError(f"{what}: first difference at {where}")
    return counts


# ------------------------------------------------------------------ 1. entry search
@pytest.mark.parametrize("kind", bs.KINDS)
def test_entry_search_with_empty_entries_and_gaps(kind):
    t = bs.entry_search_case(kind, 300, "runs", 1)
    runs, lead, trail = bs.empty_runs(t)
    assert lead and trail and {1, 2, 5} <= set(runs) and t.n_tiles() > 300
    check(t, f"{kind}, 300 entries")


@pytest.mark.parametrize("n", SEARCH_SIZES)
@pytest.mark.parametrize("kind", bs.KINDS)
def test_entry_search_by_table_size(kind, n):
    for layout in layouts_of(n):
        t = bs.entry_search_case(kind, n, layout, 2)
        assert len(t.entries) == n
        check(t, f"{kind}, {n} entries, {layout}")


# ------------------------------------------------------------------ 2. scalar skip
@pytest.mark.parametrize("wide_q", [False, True], ids=["Q1", "Q4"])
def test_submodel_scalar_skip_on_tile_boundaries(wide_q):
    t = bs.scalar_skip_submodel(wide_q)
    assert {v[1] * v[2] for v in t.views} == set(bs.SKIP_ROWS) and {bs.TILE, 2 * bs.TILE} <= set(bs.leading_ends(t))
    counts = check(t, "submodel skip")
    assert counts.max() == 2 and counts.min() == 0


@pytest.mark.parametrize("n_dims", [1, 2, 3, 4])
def test_elastic_scalar_skip_on_tile_boundaries(n_dims):
    t = bs.scalar_skip_elastic(n_dims)
    assert {bs.TILE, 2 * bs.TILE} <= set(bs.leading_ends(t))
    assert n_dims == 1 or {bs.TILE % prod(v[5 - n_dims:]) == 0 for v in t.views} == {False, True}
    counts = check(t, f"elastic skip, {n_dims} dims")
    assert counts.max() == 2 and counts.min() == 0


# ------------------------------------------------------------------ 3. ballot skip
@pytest.mark.parametrize("kind,rows", [("submodel", False), ("submodel", True), ("elastic", False)],
                         ids=["submodel", "submodel-rows", "elastic"])
def test_ballot_skip_on_wave_boundaries(kind, rows):
    t = bs.ballot_case(kind, rows)
    assert len(t.views) == len(bs.BALLOT_PREFIXES) + len(bs.BALLOT_ROWS) * len(bs.BALLOT_CUTS)
    counts = check(t, f"{kind} ballot")
    assert counts.max() == 2 and counts.min() == 0


# ------------------------------------------------------------------ 4. elastic view patterns
@pytest.mark.parametrize("pattern", range(16), ids=[f"{p:04b}"[::-1] for p in range(16)])
def test_elastic_view_patterns(pattern):
    t = bs.view_pattern_case(pattern)
    assert [v != 1 for v in t.views[0]] == [bool(pattern >> d & 1) for d in range(4)]
    counts = check(t, f"view {t.views[0]}")
    assert counts.max() == 3  # the boxes with an extent of 0 add nothing


# ------------------------------------------------------------------ 5. K at the limit
@pytest.mark.parametrize("kind", bs.KINDS)
def test_4096_clients(kind):
    t = bs.k_limit_case(kind)
    assert t.k == _lib.PLATO_AGG_SUBMODEL_MAX_K == 4096 and len(t.entry_boxes(0)) == 4096
    counts = check(t, f"{kind}, K = 4096")
    assert counts.max() == 4096 and counts[t.offset(0):t.offset(0) + 1025].min() == 1024


# ------------------------------------------------------------------ 6. fuzz
@pytest.mark.parametrize("kind", bs.KINDS)
def test_seeded_fuzz(kind):
    for seed in bs.FUZZ_SEEDS:
        check(bs.fuzz_case(kind, seed), f"{kind} fuzz, seed {seed}")


# ------------------------------------------------------------------ 7. the 64-bit path
WIDE_BYTES = 14 << 30  # g, out and the shared client buffer at 4.34 GB each, and room for the gathers


@pytest.mark.parametrize("kind", bs.KINDS)
def test_entries_of_2_30_elements_and_more(kind):
    """One entry of a little over 2^30 elements under each view, three boxes (cut on every dim, half of the
    leading dim, tiny), checked at about 2^20 sampled elements against the per-element form."""
    views = bs.WIDE_VIEWS[kind]
    if torch.cuda.mem_get_info(DEV)[0] < WIDE_BYTES:
        pytest.skip("less than 14 GiB of device memory free")
    n_max = max(prod(v) for v in views)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(7)
    g = shared = small = out = None
    try:
        g = torch.randn(bs.WIDE_LEAD + n_max, generator=gen, device=DEV, dtype=torch.float32)
        shared = torch.randn(max(bs.wide_row_len(v)[0] for v in views), generator=gen, device=DEV, dtype=torch.float32)
        small = torch.randn(max(bs.wide_row_len(v)[2] for v in views), generator=gen, device=DEV, dtype=torch.float32)
        out = torch.empty(bs.WIDE_LEAD + n_max + GUARD, dtype=torch.float32, device=DEV)
        table = torch.tensor([shared.data_ptr(), shared.data_ptr(), small.data_ptr()], dtype=torch.int64, device=DEV)
        for view in views:
            n = prod(view)
            assert n >= 1 << 30
            entries, boxes, row_len = bs.wide_tables(kind, view)
            assert row_len[0] <= shared.numel() and row_len[2] <= small.numel()
            n_out = bs.WIDE_LEAD + n
            out.fill_(SENTINEL)
            nbytes, work = workspace(kind, 3, 1, 3)
            mean(kind, g, table, 3, row_len, entries, boxes, work, out, n_out)

            sample = bs.wide_sample(view, 7)
            at = torch.from_numpy(sample + bs.WIDE_LEAD).to(DEV)
            got, gv = out[at].cpu().numpy(), g[at].cpu().numpy()
            cover = bs.wide_cover(view, sample)
            xs = [buf[torch.from_numpy(idx + src).to(DEV)].cpu().numpy()  # where not covered: the box's first element
                  for (_, idx), src, buf in zip(cover, bs.WIDE_SRC, (shared, shared, small))]
            want, counts = bs.combine(gv, xs, [c for c, _ in cover])
            bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
            assert not bad.size, (f"{kind} {view}: {bad.size} of {sample.size} sampled elements differ, the first "
                                  f"at flat index {int(sample[bad[0]])} (count {int(counts[bad[0]])})")
            # what the sample holds, from the host's counts
            assert set(np.unique(counts)) == {0, 1, 2, 3}
            pairs = sum(int(c.sum()) for c, _ in cover)
            above = sum(int((c & (idx >= (1 << 30))).sum()) for c, idx in cover)
            if prod(bs.wide_boxes(view)[0]) > 1 << 30:
                assert 4 * above >= pairs
            else:  # four dims: no box of three cut ones reaches 2^30 elements (tests/box_seams.py)
                assert 4 * int((sample >= 1 << 30).sum()) >= sample.size
            # nothing written in front of the entry or behind it, nor behind the workspace
            assert bool((out[:bs.WIDE_LEAD] == SENTINEL).all()) and bool((out[n_out:] == SENTINEL).all())
            assert bool((work[nbytes:] == PAD).all())
    finally:
        del g, shared, small, out
        torch.cuda.empty_cache()
