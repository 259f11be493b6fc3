"""The tables and restatements of tests/box_seams.py, on the CPU: the two restatements agree on every case the
GPU tests run below 2^30 elements, the tables have the properties those tests rely on (read from the tables),
the restatement agrees with tests/submodel_oracle.py and tests/elastic_oracle.py on a toy case each, and the
sample of the 64-bit tests holds what they claim, by the reference alone."""

from math import prod

import numpy as np
import pytest

from plato_amd import _lib
from tests import box_seams as bs
from tests import elastic_cases as ec
from tests import elastic_oracle as eo
from tests import submodel_cases as sc
from tests import submodel_oracle as so


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def narrow_cases():
    """(name, thunk) of every case of sections 1 to 6 of the GPU tests."""
    out = []
    for kind in bs.KINDS:
        out.append((f"search-{kind}-runs", lambda kind=kind: bs.entry_search_case(kind, 300, "runs", 1)))
        for n in SEARCH_SIZES:
            for layout in layouts_of(n):
                out.append((f"search-{kind}-{n}-{layout}",
                            lambda kind=kind, n=n, layout=layout: bs.entry_search_case(kind, n, layout, 2)))
        out.append((f"limit-{kind}", lambda kind=kind: bs.k_limit_case(kind)))
        for seed in bs.FUZZ_SEEDS:
            out.append((f"fuzz-{kind}-{seed}", lambda kind=kind, seed=seed: bs.fuzz_case(kind, seed)))
    out += [("skip-submodel-q1", lambda: bs.scalar_skip_submodel(False)),
            ("skip-submodel-q4", lambda: bs.scalar_skip_submodel(True)),
            ("ballot-submodel", lambda: bs.ballot_case("submodel")),
            ("ballot-submodel-rows", lambda: bs.ballot_case("submodel", True)),
            ("ballot-elastic", lambda: bs.ballot_case("elastic"))]
    out += [(f"skip-elastic-{n}", lambda n=n: bs.scalar_skip_elastic(n)) for n in (1, 2, 3, 4)]
    out += [(f"pattern-{p:04b}", lambda p=p: bs.view_pattern_case(p)) for p in range(16)]
    return out


SEARCH_SIZES = (1, 2, 3, 4, 5, 255, 256, 257)


def layouts_of(n):
    return ("dense",) + (("lead", "trail") if n >= 2 else ()) + (("both",) if n >= 3 else ())


def check_tables(t: bs.Tables):
    """What both entry points check of a table, restated: ranges in order, first tiles, boxes inside rows."""
    end = tiles = listed = 0
    for e, view in enumerate(t.views):
        n = prod(view)
        assert t.offset(e) >= end and t.tile0(e) == tiles
        end, tiles = t.offset(e) + n, tiles + -(-n // bs.TILE)
        if t.kind == "elastic":
            assert int(t.entries[e, 6]) == listed
            listed += int(t.entries[e, 7])
        clients = [c for _, _, c in t.entry_boxes(e)]
        assert clients == sorted(set(clients))
        for ext, src, c in t.entry_boxes(e):
            assert all(0 <= x <= v for x, v in zip(ext, view))
            assert src % 2 == 1 and src + prod(ext) < t.row_len[c] == len(t.rows[c])  # src inside the row, odd
    assert end <= t.n_out and tiles == t.n_tiles()
    assert t.kind == "submodel" or listed == len(t.boxes)


def test_tile_is_the_librarys():
    assert bs.TILE == _lib.PLATO_AGG_SUBMODEL_TILE == _lib.PLATO_AGG_ELASTIC_TILE
    assert bs.ABSENT == _lib.PLATO_AGG_SUBMODEL_ABSENT
    assert bs.MAX_K == _lib.PLATO_AGG_SUBMODEL_MAX_K == _lib.PLATO_AGG_ELASTIC_MAX_K
    assert _lib.PLATO_AGG_SUBMODEL_ENTRY_WORDS == 6 and _lib.PLATO_AGG_SUBMODEL_BOX_WORDS == 4
    assert _lib.PLATO_AGG_ELASTIC_ENTRY_WORDS == 8 and _lib.PLATO_AGG_ELASTIC_BOX_WORDS == 6


def test_the_two_restatements_agree_on_every_narrow_case():
    for name, make in narrow_cases():
        t = make()
        check_tables(t)
        want, counts = bs.restate(t)
        again, counts2 = bs.per_element(t)
        assert bits(want).tobytes() == bits(again).tobytes(), (name, bs.first_difference(t, again, want))
        assert counts.tobytes() == counts2.tobytes(), name


def test_source_index_on_python_ints_is_the_array_form():
    rng = np.random.default_rng(5)
    for view, ext in [((7, 1, 13), (3, 1, 5)), ((1, 5, 1, 9), (1, 2, 0, 9)), ((3, 4, 5, 6), (2, 4, 1, 6))]:
        f = np.arange(prod(view), dtype=np.int64)
        c, at = bs.source_index(view, ext, f)
        c = np.broadcast_to(c, f.shape)
        for x in rng.integers(0, f.size, size=40):
            ci, ai = bs.source_index(view, ext, int(x))
            assert isinstance(ai, int) and ci == c[x] and (not ci or ai == at[x])
            if ci:
                assert bs.flat_of(view, ext, ai) == x


# ------------------------------------------------------------------ 1. entry search
def test_entry_search_tables_have_empty_entries_where_promised():
    for kind in bs.KINDS:
        t = bs.entry_search_case(kind, 300, "runs", 1)
        runs, lead, trail = bs.empty_runs(t)
        assert lead == 1 and trail == 1 and {1, 2, 5} <= set(runs)
        assert {t.numel(e) for e in range(300)} == set(bs.COUNTS)
        for e, view in enumerate(t.views):
            assert t.numel(e) or sorted(view).count(0) == 1  # an empty entry has one extent of 0
        offs = [t.offset(e) - (t.offset(e - 1) + t.numel(e - 1)) for e in range(1, 300)]
        assert min(offs) == 0 and max(offs) > 0  # gaps between some entries
        # empty entries share the first tile of the entry behind them; those at the end have the tile count
        for e in range(299):
            if not t.numel(e):
                assert t.tile0(e) == t.tile0(e + 1)
        assert t.tile0(299) == t.n_tiles()
        _, counts = bs.restate(t)
        single = set()
        for e in range(300):
            c = counts[t.offset(e):t.offset(e) + t.numel(e)]
            if c.size > 1:
                assert c.min() == 0 and c.max() >= 1, e  # a covered and an uncovered element
            elif c.size:
                single.add(int(c[0]))
        assert single == {0, 1}  # an entry of one element is one or the other: both occur
        if kind == "elastic":
            listed = {bool(t.entries[e, 7]) for e in range(300) if not t.numel(e)}
            assert listed == {False, True}  # empty entries with boxes and without
        for n in SEARCH_SIZES:
            for layout in layouts_of(n):
                s = bs.entry_search_case(kind, n, layout, 2)
                runs, lead, trail = bs.empty_runs(s)
                assert len(s.views) == n and (lead, trail) == (layout in ("lead", "both"), layout in ("trail", "both"))
                assert not runs


# ------------------------------------------------------------------ 2. scalar skip
def test_scalar_skip_tables_end_on_before_and_after_every_tile_boundary():
    for wide_q in (False, True):
        t = bs.scalar_skip_submodel(wide_q)
        assert all((v[1] == 1) != wide_q for v in t.views)
        ends = bs.leading_ends(t)
        for ql in bs.SKIP_ROWS:
            mine = {x for x, v in zip(ends, t.views) if v[1] * v[2] == ql}
            assert mine == set(range(0, 3 * bs.TILE + 1, ql))  # every p in 0..P
            for edge in (bs.TILE, 2 * bs.TILE):
                on = {edge - ql, edge, edge + ql} <= mine
                assert on == (bs.TILE % ql == 0 or ql == bs.TILE), ql
            if ql == 1536:  # the straddling rows: a box ends inside the second tile and nowhere on its edges
                assert 1536 in mine and not mine & {1024, 2048}
    for n_dims in (1, 2, 3, 4):
        t = bs.scalar_skip_elastic(n_dims)
        assert all(v[:4 - n_dims] == (1,) * (4 - n_dims) and v[4 - n_dims] != 1 for v in t.views)
        ends = bs.leading_ends(t)
        inners = sorted({prod(v[5 - n_dims:]) for v in t.views})
        assert inners == ([1] if n_dims == 1 else sorted(prod(i) for i in bs.ELASTIC_INNER[n_dims]))
        for inner in inners:
            mine = {x for x, v in zip(ends, t.views) if prod(v[5 - n_dims:]) == inner}
            for edge in (bs.TILE, 2 * bs.TILE):
                if bs.TILE % inner == 0:
                    assert {edge - inner, edge, edge + inner} <= mine, (n_dims, inner)
                else:  # the nearest rows either side
                    assert edge not in mine and {edge // inner * inner, (edge // inner + 1) * inner} <= mine
        if n_dims > 1:
            assert [bs.TILE % i == 0 for i in inners] == [False, True]  # 77 or 105, and 256
            # the extents behind the compared dim are all above 1: a kernel that took fewer of them for
            # `inner` would compare another row count
            assert all(min(v[5 - n_dims:]) > 1 for v in t.views)


# ------------------------------------------------------------------ 3. ballot skip
def test_ballot_tables_split_waves_in_every_stride():
    for kind, rows in (("submodel", False), ("submodel", True), ("elastic", False)):
        t = bs.ballot_case(kind, rows)
        n1 = len(bs.BALLOT_PREFIXES)
        assert [t.numel(e) for e in range(n1)] == [bs.BALLOT_N] * n1
        assert tuple(t.entry_boxes(e)[0][0][-1] for e in range(n1)) == bs.BALLOT_PREFIXES
        mixed_strides, late_only = set(), 0
        for e in range(len(t.views)):
            cover = bs.lane_cover(t.views[e], t.entry_boxes(e)[0][0])
            some, every = cover.any(axis=3), cover.all(axis=3)
            for h in range(4):
                if (some[:, :, h] & ~every[:, :, h]).any():
                    mixed_strides.add(h)  # a wave with covered and uncovered lanes in stride h
            if e >= n1:
                late_only += int((~some[:, :, 0] & some[:, :, 1:].any(axis=2)).sum())
            else:  # a prefix on a wave boundary: some wave is covered in full and the next not at all
                l = bs.BALLOT_PREFIXES[e]
                if l % bs.WAVE == 0 and l < bs.BALLOT_N:
                    flat_some = some.transpose(0, 2, 1).reshape(-1)  # in element order: tile, stride, wave
                    assert flat_some[l // bs.WAVE - 1] and not flat_some[l // bs.WAVE]
        assert mixed_strides == {0, 1, 2, 3}
        assert late_only > 0  # waves that stride 0 alone would skip although another stride is covered


# ------------------------------------------------------------------ 4. view patterns
def test_view_patterns_are_all_sixteen_with_every_empty_box():
    seen = set()
    for p in range(16):
        t = bs.view_pattern_case(p)
        view = t.views[0]
        seen.add(tuple(v != 1 for v in view))
        n = prod(view)
        assert (n == 1) if p == 0 else (1024 < n <= 4096)
        assert all(v % 2 == 1 for v in view)
        exts = [b[0] for b in t.entry_boxes(0)]
        assert exts[0] == view and exts[2] == (1, 1, 1, 1)
        assert all((c == v - 1) if v > 1 else c == 1 for c, v in zip(exts[1], view))
        zeros = exts[3:]
        assert len(zeros) == sum(v == 1 for v in view)
        for z in zeros:
            d = z.index(0)
            assert view[d] == 1 and all(x == v for i, (x, v) in enumerate(zip(z, view)) if i != d)
        lead = next((d for d, v in enumerate(view) if v != 1), 3)
        assert {z.index(0) for z in zeros} >= set(range(lead))  # every leading dim the kernel's `empty` names
        _, counts = bs.restate(t)
        c = counts[t.offset(0):t.offset(0) + n]
        assert c.max() == 3 and (p == 0 or c.min() == 1)
    assert len(seen) == 16


# ------------------------------------------------------------------ 5. K at the limit
def test_k_limit_counts_reach_4096_exactly():
    for kind in bs.KINDS:
        t = bs.k_limit_case(kind)
        assert t.k == 4096 and t.numel(0) == 1025 and len(t.entry_boxes(0)) == 4096
        assert [c for _, _, c in t.entry_boxes(0)] == list(range(4096))
        _, counts = bs.restate(t)
        c = counts[t.offset(0):t.offset(0) + 1025]
        assert c.max() == 4096 and c.min() == 1024 and np.float32(4096) == 4096
        assert len({b[0] for b in t.entry_boxes(0)}) == 4


# ------------------------------------------------------------------ 6. fuzz
def test_fuzz_cases_cover_what_they_should():
    for kind in bs.KINDS:
        ks, ns, ranks, kinds_of_box = set(), [], set(), set()
        for seed in bs.FUZZ_SEEDS:
            t = bs.fuzz_case(kind, seed)
            assert 1 <= len(t.views) <= 12 and 1 <= t.k <= 9
            ks.add(t.k)
            for e, view in enumerate(t.views):
                assert prod(view) <= bs.FUZZ_MAX_N
                ns.append(prod(view))
                ranks.add(sum(v != 1 for v in view))
                held = t.entry_boxes(e)
                kinds_of_box.add("absent" if len(held) < t.k else "all")
                for ext, _, _ in held:
                    kinds_of_box.add("full" if ext == view else "zero" if not prod(ext) else "part")
        assert len(bs.FUZZ_SEEDS) == 100 and ks == set(range(1, 10))
        assert kinds_of_box == {"absent", "all", "full", "zero", "part"}
        assert ranks >= set(range(1, bs.RANK[kind] + 1)) and max(ns) > 4 * bs.TILE and 0 in ns


# ------------------------------------------------------------------ the oracles
def submodel_description(g, clients, rule):
    views, boxes = [], []
    for name, a in g.items():
        if not so.participates(name):
            continue
        r = so.rank_of(rule, a.ndim)

        def seen(shape):
            lead = tuple(shape[:r]) + (1,) * (2 - min(r, 2))
            return (*lead[:2], prod(shape[2:])) if r < 3 else tuple(shape)
        views.append(seen(a.shape) if r else (1, 1, a.size))
        boxes.append([seen(c[name].shape) if r else None for c in clients])
    return views, boxes


def elastic_description(g, clients):
    views, boxes = [], []
    for name, a in g.items():
        r = eo.rank_of(name, a.ndim)
        views.append((1,) * (4 - r) + tuple(a.shape) if r else (1, 1, 1, a.size))
        boxes.append([(1,) * (4 - r) + tuple(c[name].shape) if r and name in c else None for c in clients])
    return views, boxes


def with_models(t: bs.Tables, g, clients, names):
    """The tables' values replaced by the models': g's entries into gflat, every client's tensors into its row."""
    for e, name in enumerate(names):
        t.gflat[t.offset(e):t.offset(e) + t.numel(e)] = g[name].reshape(-1)
        for ext, src, c in t.entry_boxes(e):
            t.rows[c][src:src + prod(ext)] = clients[c][name].reshape(-1)
    return t


@pytest.mark.parametrize("rule", ["heterofl", "fedrolex"])
def test_restatement_is_the_submodel_oracle_on_the_toy_case(rule):
    rates = (0.5, 0.125, 1.0, 0.25, 0.5)
    g = sc.fill(sc.toy_spec(1.0), 7, 0)
    clients = [sc.fill(sc.toy_spec(r), 7, 1 + k) for k, r in enumerate(rates)]
    names = [n for n in g if so.participates(n)]
    t = with_models(bs.build("submodel", *submodel_description(g, clients, rule)), g, clients, names)
    want, counts = so.aggregate(g, clients, rule)
    for kernel in (bs.restate, bs.per_element):
        got, cnt = kernel(t)
        for e, name in enumerate(names):
            at = slice(t.offset(e), t.offset(e) + t.numel(e))
            assert bits(got[at]).tobytes() == bits(want[name]).tobytes(), name
            assert cnt[at].tobytes() == counts[name].reshape(-1).tobytes(), name
    assert any(c.max() == 5 for c in counts.values()) and any(c.min() == 0 for c in counts.values())


def test_restatement_is_the_elastic_oracle_on_the_toy_case():
    g = sc.fill(ec.toy_spec(ec.TOY_GLOBAL), 7, 0)
    clients = [sc.fill(ec.toy_spec(cfg), 7, 1 + k) for k, cfg in enumerate(ec.TOY_CLIENTS)]
    g = {n: a for n, a in g.items() if a.dtype == np.float32}
    names = list(g)
    t = with_models(bs.build("elastic", *elastic_description(g, clients)), g, clients, names)
    want, counts = eo.aggregate(g, clients)
    for kernel in (bs.restate, bs.per_element):
        got, cnt = kernel(t)
        for e, name in enumerate(names):
            at = slice(t.offset(e), t.offset(e) + t.numel(e))
            assert bits(got[at]).tobytes() == bits(want[name]).tobytes(), name
            assert cnt[at].tobytes() == counts[name].reshape(-1).tobytes(), name
    assert any(c.size and c.min() == 0 for c in counts.values()) and max(c.max() for c in counts.values() if c.size) >= 2


# ------------------------------------------------------------------ 7. the 64-bit path, by the reference alone
@pytest.mark.parametrize("kind", bs.KINDS)
def test_wide_views_and_samples_hold_what_the_gpu_test_claims(kind):
    for view in bs.WIDE_VIEWS[kind]:
        n = prod(view)
        assert (1 << 30) <= n <= (1 << 30) * 101 // 100
        assert all(v == 1 or v & (v - 1) for v in view)  # no extent is a power of two
        cut, half, tiny = bs.wide_boxes(view)
        assert all(1 <= v - c <= 3 if v != 1 else c == 1 for v, c in zip(view, cut))
        lead = next(d for d, v in enumerate(view) if v != 1)
        assert half[lead] == view[lead] // 2 + 1 and half[:lead] + half[lead + 1:] == view[:lead] + view[lead + 1:]
        assert prod(half) % bs.TILE and prod(tiny) <= 210  # the skip flips off a tile boundary
        row_len = bs.wide_tables(kind, view)[2]
        for ext, src, length in zip(bs.wide_boxes(view), bs.WIDE_SRC, row_len):
            assert src % 2 == 1 and src + prod(ext) < length
        assert row_len[0] == row_len[1]

        sample = bs.wide_sample(view, 7)
        assert sample[0] == 0 and sample[-1] == n - 1 and (np.diff(sample) > 0).all()
        # 2^20 draws; those that repeat (the tail is a few million elements) are kept once
        assert (1 << 20) * 7 // 8 <= sample.size <= (1 << 20) + 6 * 2048
        for edge in (0, n - 2048, prod(half) - 2048, (1 << 30) - 2048):
            at = np.searchsorted(sample, edge)
            assert (sample[at:at + 2048] == np.arange(edge, edge + 2048)).all()
        cover = bs.wide_cover(view, sample)
        counts = sum(c.astype(np.int32) for c, _ in cover)
        assert set(np.unique(counts)) == {0, 1, 2, 3}
        pairs = sum(int(c.sum()) for c, _ in cover)
        above = sum(int((c & (at >= (1 << 30))).sum()) for c, at in cover)
        if prod(cut) > (1 << 30):
            assert 4 * above >= pairs, (view, above, pairs)
        else:
            # (37, 29, 1009, 997): a cut on four dims leaves fewer than 2^30 elements, whatever the extents of
            # an entry this size, so no source index passes 2^30; a quarter of the sample's elements lie at
            # flat indices from 2^30 on instead
            assert len([v for v in view if v != 1]) == 4 and above == 0
            assert 4 * int((sample >= (1 << 30)).sum()) >= sample.size
        # the array form against Python ints on a part of the sample
        for x in sample[:: sample.size // 1024]:
            for ext, (c, at) in zip(bs.wide_boxes(view), cover):
                ci, ai = bs.source_index(view, ext, int(x))
                i = np.searchsorted(sample, x)
                assert ci == c[i] and (not ci or ai == at[i])
