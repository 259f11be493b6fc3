"""Tables and restatements for the seams of the two box kernels, plato_agg_submodel_mean (csrc/submodel.hip)
and plato_agg_elastic_mean (csrc/elastic.hip): the entry search, the scalar skip on tile boundaries, the
ballot skip on wave boundaries, views with extents of 1, K at the ABI's limit, a seeded fuzz and the entries
of 2^30 elements and more that take the 64-bit index path.  No GPU and no torch in here: tests/test_box_seams.py
checks these tables and restatements on the CPU, tests/test_box_seams_gpu.py runs the kernels on them.

A case is a description: a list of entry views ([P, Q, L] for "submodel", (A, B, C, D) for "elastic"), and per
entry one leading-corner box (a tuple of extents) or None (absent) per client.  `build` turns it into the
ABI's tables.  Every client row starts with one float nobody reads, every box starts at an odd offset of its
row and every row ends with one more float, so every `src`, that of a box of zero elements included, lies
inside the row: a kernel that failed to skip a box gives a wrong number and reads nothing outside a buffer.
`pack_rows` puts the rows at odd offsets of one array, which the GPU tests upload once.

Two restatements, written apart from each other:
  * `restate`: per entry, numpy slices of the reshaped arrays in table order, the arithmetic of the direct-call
    tests of tests/test_submodel_gpu.py and tests/test_elastic_gpu.py (acc = g; acc = acc + x per covering
    box, float32; (acc - g) / max(cnt, 1)), written into a sentinel-filled output;
  * `source_index` and `per_element`: an element's coordinates from its flat index by `//` and `%`, the box's
    source index from them.  `source_index` takes a Python int (no width at all) or an int64 array (every
    product here stays below 2^31, so int64 is exact); the CPU tests hold the two against each other.
"""

from __future__ import annotations

from dataclasses import dataclass
from math import prod

import numpy as np

TILE = 1024      # PLATO_AGG_SUBMODEL_TILE == PLATO_AGG_ELASTIC_TILE (tests/test_box_seams.py compares)
THREADS = 256    # lanes of a workgroup; a lane owns TILE / THREADS elements THREADS apart
WAVE = 64
ABSENT = -1
MAX_K = 4096
SENTINEL = np.float32(-7.0)
F32 = np.float32
KINDS = ("submodel", "elastic")
RANK = {"submodel": 3, "elastic": 4}
NARROW = 1 << 30  # entries of this many elements and more are indexed in 64 bits


# ------------------------------------------------------------------ tables
@dataclass
class Tables:
    kind: str
    views: list          # per entry, a tuple of RANK[kind] extents
    entries: np.ndarray  # int64 [E, 6] or [E, 8]
    boxes: np.ndarray    # int64 [E, K, 4] or [n_boxes, 6]
    row_len: np.ndarray  # int64 [K]
    rows: list           # K float32 arrays
    gflat: np.ndarray    # float32 [n_out]
    n_out: int
    k: int

    def numel(self, e: int) -> int:
        return prod(self.views[e])

    def offset(self, e: int) -> int:
        return int(self.entries[e, 0])

    def tile0(self, e: int) -> int:
        return int(self.entries[e, 4 if self.kind == "submodel" else 5])

    def n_tiles(self) -> int:
        return sum(-(-self.numel(e) // TILE) for e in range(len(self.views)))

    def entry_boxes(self, e: int):
        """[(extents, src, client)] of entry e in table order, read from the ABI tables."""
        if self.kind == "submodel":
            return [(tuple(int(v) for v in b[:3]), int(b[3]), c) for c, b in enumerate(self.boxes[e]) if b[3] >= 0]
        first, n = int(self.entries[e, 6]), int(self.entries[e, 7])
        return [(tuple(int(v) for v in b[:4]), int(b[4]), int(b[5])) for b in self.boxes[first:first + n]]


def build(kind: str, views, boxes, gaps=None, seed: int = 0, lead: int = 3, tail: int = 5) -> Tables:
    """The tables of a description.  `gaps[e]` output elements lie unused in front of entry e (after `lead` in
    front of everything); `tail` more follow the last entry."""
    rank = RANK[kind]
    views = [tuple(int(v) for v in view) for view in views]
    k = len(boxes[0])
    assert all(len(v) == rank for v in views) and all(len(b) == k for b in boxes) and len(boxes) == len(views)
    gaps = [0] * len(views) if gaps is None else list(gaps)
    cursor = [1] * k  # the next free element of each client's row: odd
    ent, box_rows, off, tile = [], [], lead, 0
    for e, view in enumerate(views):
        n = prod(view)
        off += gaps[e]
        listed = []
        for c, ext in enumerate(boxes[e]):
            if ext is None:
                if kind == "submodel":
                    listed.append([0, 0, 0, ABSENT])
                continue
            ext = tuple(int(v) for v in ext)
            assert len(ext) == rank and all(0 <= x <= v for x, v in zip(ext, view)), (e, c, ext, view)
            listed.append([*ext, cursor[c]] + ([c] if kind == "elastic" else []))
            cursor[c] += prod(ext)
            cursor[c] += 1 - cursor[c] % 2
        if kind == "submodel":
            ent.append([off, *view, tile, 0])
            box_rows.append(listed)
        else:
            ent.append([off, *view, tile, len(box_rows), len(listed)])
            box_rows.extend(listed)
        off += n
        tile += -(-n // TILE)
    n_out = off + tail
    entries = np.array(ent, dtype=np.int64).reshape(len(views), 6 if kind == "submodel" else 8)
    table = np.array(box_rows, dtype=np.int64).reshape((len(views), k, 4) if kind == "submodel" else (-1, 6))
    row_len = np.array([c + 1 for c in cursor], dtype=np.int64)
    rng = np.random.default_rng([seed, 0x5EA])
    gflat = rng.standard_normal(n_out).astype(F32)
    flat = rng.standard_normal(int(row_len.sum())).astype(F32)
    rows = np.split(flat, np.cumsum(row_len)[:-1])
    return Tables(kind, views, entries, table, row_len, rows, gflat, n_out, k)


def pack_rows(rows):
    """(one float32 array, the odd element offset of every row in it)."""
    starts, cursor = [], 1
    for r in rows:
        starts.append(cursor)
        cursor += len(r)
        cursor += 1 - cursor % 2
    flat = np.zeros(cursor + 1, dtype=F32)
    for s, r in zip(starts, rows):
        flat[s:s + len(r)] = r
    return flat, starts


# ------------------------------------------------------------------ the slice restatement
def restate(t: Tables):
    """(the output region, sentinel where no entry lies; the count per output element, 0 there)."""
    want = np.full(t.n_out, SENTINEL, dtype=F32)
    counts = np.zeros(t.n_out, dtype=np.int32)
    for e, view in enumerate(t.views):
        off, n = t.offset(e), t.numel(e)
        gv = t.gflat[off:off + n].reshape(view)
        acc, cnt = gv.copy(), np.zeros(view, dtype=np.int32)
        for ext, src, client in t.entry_boxes(e):
            at = tuple(slice(0, x) for x in ext)
            acc[at] = acc[at] + t.rows[client][src:src + prod(ext)].reshape(ext)
            cnt[at] += 1
        want[off:off + n] = ((acc - gv) / np.maximum(cnt, 1).astype(F32)).reshape(-1)
        counts[off:off + n] = cnt.reshape(-1)
    return want, counts


# ------------------------------------------------------------------ the per-element form
def source_index(view, ext, f):
    """(covered, index into the box's elements) of the element with flat index f of an entry seen as `view`,
    for the leading-corner box `ext`.  f: a Python int, or an int64 array; the index of an element that is
    not covered means nothing."""
    coords, rem = [], f
    for v in reversed(view):
        coords.append(rem % v)
        rem = rem // v
    covered, at = True, 0
    for x, b in zip(reversed(coords), ext):
        covered = covered & (x < b)
        at = at * b + x
    return covered, at


def flat_of(view, ext, at: int) -> int:
    """The flat index in `view` of element `at` of the box `ext` (Python ints)."""
    coords = []
    for b in reversed(ext):
        coords.append(at % b)
        at //= b
    f = 0
    for x, v in zip(reversed(coords), view):
        f = f * v + x
    return f


def combine(g: np.ndarray, xs, covers):
    """(acc - g) / max(cnt, 1) with acc = g, then acc + x where covered, in order, float32; and cnt."""
    acc, cnt = g.astype(F32, copy=True), np.zeros(g.shape, dtype=np.int32)
    for x, c in zip(xs, covers):
        acc = np.where(c, acc + x.astype(F32, copy=False), acc)
        cnt += c
    return (acc - g) / np.maximum(cnt, 1).astype(F32), cnt


def per_element(t: Tables):
    """What `restate` returns, from flat indices alone."""
    want = np.full(t.n_out, SENTINEL, dtype=F32)
    counts = np.zeros(t.n_out, dtype=np.int32)
    for e, view in enumerate(t.views):
        off, n = t.offset(e), t.numel(e)
        if not n:
            continue
        f = np.arange(n, dtype=np.int64)
        xs, covers = [], []
        for ext, src, client in t.entry_boxes(e):
            c, at = source_index(view, ext, f)
            c = np.broadcast_to(c, f.shape)
            covers.append(c)
            xs.append(t.rows[client][src + np.where(c, at, 0)])
        want[off:off + n], counts[off:off + n] = combine(t.gflat[off:off + n], xs, covers)
    return want, counts


def first_difference(t: Tables, got: np.ndarray, want: np.ndarray):
    """None, or (entry or None, flat index in it or in the region) of the first element whose bits differ."""
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    if not bad.size:
        return None
    at = int(bad[0])
    for e in range(len(t.views)):
        if t.offset(e) <= at < t.offset(e) + t.numel(e):
            return e, at - t.offset(e)
    return None, at


def lane_cover(view, ext):
    """bool [tiles, waves, strides, lanes]: which lane of which wave covers its element of each stride, as the
    kernels hand elements out (element base + lane + stride * THREADS of a tile; past the entry: False)."""
    n = prod(view)
    tiles = -(-n // TILE)
    f = (np.arange(tiles, dtype=np.int64)[:, None, None, None] * TILE
         + np.arange(THREADS // WAVE, dtype=np.int64)[None, :, None, None] * WAVE
         + np.arange(TILE // THREADS, dtype=np.int64)[None, None, :, None] * THREADS
         + np.arange(WAVE, dtype=np.int64)[None, None, None, :])
    c, _ = source_index(view, ext, np.minimum(f, n - 1))
    return np.broadcast_to(c, f.shape) & (f < n)


# ------------------------------------------------------------------ 1. entry search
COUNTS = (0, 1, 1023, 1024, 1025, 2049)
VIEWS_OF = {  # per count, views of rank 4; the submodel ones are those that start with 1, without it
    1: [(1, 1, 1, 1)],
    1023: [(1, 3, 11, 31), (1, 1, 33, 31), (1, 1, 1, 1023), (3, 11, 1, 31), (1, 31, 1, 33), (3, 1, 11, 31)],
    1024: [(1, 4, 8, 32), (1, 1, 32, 32), (1, 1, 1, 1024), (2, 4, 8, 16), (1, 16, 1, 64), (4, 8, 32, 1)],
    1025: [(1, 5, 5, 41), (1, 1, 25, 41), (1, 1, 1, 1025), (5, 5, 1, 41), (1, 41, 1, 25), (5, 1, 5, 41)],
    2049: [(1, 3, 1, 683), (1, 1, 3, 683), (1, 1, 1, 2049), (3, 1, 1, 683), (1, 683, 3, 1), (1, 3, 683, 1)],
    0: [(1, 0, 3, 5), (1, 4, 0, 5), (1, 4, 3, 0), (0, 2, 3, 5), (1, 1, 1, 0), (1, 0, 1, 1)],
}


def _view(kind, count, rng):
    views = VIEWS_OF[count]
    if kind == "submodel":
        views = [v[1:] for v in views if v[0] == 1]
    return views[int(rng.integers(len(views)))]


def _search_boxes(kind, view, rng, e):
    """Three clients.  No box reaches the last index of the entry's largest dim, and the first covers the
    entry's first element, so an entry of more than one element has a covered and an uncovered element; an
    entry of one element is covered by its first client in every other entry of the table."""
    n = prod(view)
    if n == 0:
        zero = tuple(min(v, 1) if v else 0 for v in view)
        full = tuple(view)
        # submodel tables hold a row per client anyway; elastic empty entries list boxes in two of three
        return [[full, None, zero], [None, None, None], [zero, full, None]][e % 3]
    if n == 1:
        one = tuple(view)
        return [one if e % 2 else None, None, None]
    big = max(range(len(view)), key=lambda d: view[d])
    half = tuple(max(v // 2, 1) if d == big else v for d, v in enumerate(view))
    rand = tuple(int(rng.integers(0, v if d == big else v + 1)) for d, v in enumerate(view))
    third = None if rng.integers(2) else tuple(int(rng.integers(0, v if d == big else v + 1)) for d, v in enumerate(view))
    return [half, rand, third]


def entry_search_case(kind: str, n_entries: int, layout: str, seed: int) -> Tables:
    """`layout`: "dense" (no empty entry), "lead", "trail", "both" (the first, the last or both are empty), or
    "runs" (a few hundred entries: empty first and last, runs of 1, 2 and 5 empty entries in the middle and
    more at random)."""
    rng = np.random.default_rng([seed, n_entries, KINDS.index(kind)])
    full = [c for c in COUNTS if c]
    counts = [int(rng.choice(full)) for _ in range(n_entries)]
    if layout == "runs":
        assert n_entries >= 64
        for at in range(n_entries):
            if rng.random() < 0.1:
                counts[at] = 0
        for start, run in ((n_entries // 4, 1), (n_entries // 2, 2), (3 * n_entries // 4, 5)):
            counts[start - 1] = counts[start + run] = int(rng.choice(full))
            counts[start:start + run] = [0] * run
        counts[0] = counts[-1] = 0
        counts[1], counts[-2] = 1025, 1
    if layout in ("lead", "both"):
        counts[0] = 0
    if layout in ("trail", "both"):
        counts[-1] = 0
    assert any(counts), "a table without a tile launches nothing"
    views = [_view(kind, c, rng) for c in counts]
    boxes = [_search_boxes(kind, v, rng, e) for e, v in enumerate(views)]
    gaps = [int(rng.choice([0, 0, 1, 7])) for _ in views]
    return build(kind, views, boxes, gaps, seed)


def empty_runs(t: Tables):
    """The lengths of the runs of empty entries strictly inside the table, and whether first / last are empty."""
    empty = [t.numel(e) == 0 for e in range(len(t.views))]
    runs, run, lead, trail = [], 0, 0, 0
    while lead < len(empty) and empty[lead]:
        lead += 1
    while trail < len(empty) - lead and empty[-1 - trail]:
        trail += 1
    for x in empty[lead:len(empty) - trail]:
        if x:
            run += 1
        elif run:
            runs.append(run)
            run = 0
    return runs, lead, trail


# ------------------------------------------------------------------ 2. the scalar skip on tile boundaries
SKIP_ROWS = (256, 512, 1024, 1536)  # Q * L of the submodel cases: three divide the tile, 1,536 straddles


def scalar_skip_submodel(wide_q: bool) -> Tables:
    """Per row size one entry of three tiles per p in 0..P: client 0 holds (p, Q, L), client 1 a box cut on
    the other dims.  p * Q * L passes every tile boundary of the entry one row at a time."""
    views, boxes = [], []
    for ql in SKIP_ROWS:
        q = 4 if wide_q else 1
        view = (3 * TILE // ql, q, ql // q)
        for p in range(view[0] + 1):
            views.append(view)
            boxes.append([(p, view[1], view[2]), (view[0], max(view[1] - 1, 1), view[2] - 3)])
    return build("submodel", views, boxes, seed=200 + wide_q)


ELASTIC_INNER = {  # per N, the extents behind the compared dim: their product divides the tile, or does not
    4: [(4, 8, 8), (3, 5, 7)],
    3: [(16, 16), (7, 11)],
    2: [(256,), (77,)],
    1: [()],
}
ELASTIC_PREFIXES = (0, 1, 1023, 1024, 1025, 2047, 2048, 2049, 3071, 3072)  # N == 1: a row is one element


def scalar_skip_elastic(n_dims: int) -> Tables:
    """The same for the view dim the kernel compares when the first 4 - n_dims extents are 1: per choice of
    the extents behind it one entry of three tiles or a little more per extent 0..E of box 0 in that dim."""
    views, boxes = [], []
    for inner in ELASTIC_INNER[n_dims]:
        rows = -(-3 * TILE // prod(inner))
        view = (1,) * (4 - n_dims) + (rows,) + inner
        cut = (1,) * (4 - n_dims) + (rows,) + tuple(v - 1 for v in inner)
        for x in (ELASTIC_PREFIXES if n_dims == 1 else range(rows + 1)):
            views.append(view)
            boxes.append([(1,) * (4 - n_dims) + (x,) + inner, (1, 1, 1, 1500) if n_dims == 1 else cut])
    return build("elastic", views, boxes, seed=210 + n_dims)


def leading_ends(t: Tables, client: int = 0):
    """Per entry, where box `client`'s leading extent ends in flat elements of the entry: extent * inner."""
    ends = []
    for e, view in enumerate(t.views):
        lead = next((d for d, v in enumerate(view) if v != 1), len(view) - 1)
        ext = [b for b in t.entry_boxes(e) if b[2] == client][0][0]
        ends.append(ext[lead] * prod(view[lead + 1:]))
    return ends


# ------------------------------------------------------------------ 3. the ballot skip on wave boundaries
BALLOT_N = 2049
BALLOT_PREFIXES = (1, 63, 64, 65, 255, 256, 257, 319, 320, 321, 1023, 1024, 1025, 2048)
BALLOT_CUTS = (63, 64, 65)
BALLOT_ROWS = ((17, 128), (7, 320))  # (rows, trailing extent): 2,176 and 2,240 elements


def _as(kind, *dims):
    return (1,) * (RANK[kind] - len(dims)) + tuple(dims)


def ballot_case(kind: str, leading_rows: bool = False) -> Tables:
    """1-D entries with each prefix, then 2-D entries whose trailing extent is cut: client 0 holds the cut box,
    client 1 the upper half of the rows in full.  `leading_rows` (submodel) puts the rows in P, with Q == 1."""
    views, boxes = [], []
    for l in BALLOT_PREFIXES:
        views.append(_as(kind, BALLOT_N))
        boxes.append([_as(kind, l), _as(kind, 700)])
    for rows, width in BALLOT_ROWS:
        for cut in BALLOT_CUTS:
            two = (lambda r, w: (r, 1, w)) if leading_rows else (lambda r, w: _as(kind, r, w))
            views.append(two(rows, width))
            boxes.append([two(rows, cut), two(rows // 2, width)])
    return build(kind, views, boxes, seed=300 + leading_rows)


# ------------------------------------------------------------------ 4. elastic views with extents of 1
ODD = {0: (), 1: (2049,), 2: (33, 63), 3: (11, 13, 15), 4: (5, 7, 9, 11)}  # 1, 2,049, 2,079, 2,145, 3,465 elements


def view_pattern_case(pattern: int) -> Tables:
    """Bit d of `pattern` set: view dim d is not 1.  Boxes: full; cut by one on every dim that is not 1; one
    element; then, per view dim of 1, a box with extent 0 there and full extents elsewhere."""
    free = [d for d in range(4) if pattern >> d & 1]
    view = [1, 1, 1, 1]
    for d, v in zip(free, ODD[len(free)]):
        view[d] = v
    view = tuple(view)
    boxes = [view, tuple(v - 1 if v > 1 else 1 for v in view), (1, 1, 1, 1)]
    boxes += [tuple(0 if x == d else v for x, v in enumerate(view)) for d in range(4) if view[d] == 1]
    return build("elastic", [view], [boxes], seed=400 + pattern)


# ------------------------------------------------------------------ 5. K at the ABI's limit
LIMIT_VIEW = (1, 5, 5, 41)  # 1,025 elements
LIMIT_SHAPES = ((1, 5, 5, 41), (1, 3, 5, 41), (1, 5, 2, 41), (1, 5, 5, 17))


def k_limit_case(kind: str) -> Tables:
    cut = RANK["elastic"] - RANK[kind]
    return build(kind, [LIMIT_VIEW[cut:]], [[LIMIT_SHAPES[c % 4][cut:] for c in range(MAX_K)]], seed=500)


# ------------------------------------------------------------------ 6. fuzz
FUZZ_SEEDS = tuple(range(1000, 1100))
FUZZ_MAX_N = 5000


def fuzz_case(kind: str, seed: int) -> Tables:
    rng = np.random.default_rng([seed, KINDS.index(kind)])
    rank = RANK[kind]
    k = int(rng.integers(1, 10))
    views, boxes = [], []
    for _ in range(int(rng.integers(1, 13))):
        r = int(rng.integers(1, rank + 1))
        dims, room = [], FUZZ_MAX_N
        for _ in range(r):
            v = int(rng.integers(1, min(room, 5000 if r == 1 else 80) + 1))
            dims.append(v)
            room //= v
        view = [1] * rank
        for d, v in zip(sorted(rng.choice(rank, size=r, replace=False)), dims):
            view[d] = v
        if rng.random() < 0.05:
            view[int(rng.integers(rank))] = 0
        assert prod(view) <= FUZZ_MAX_N
        row = []
        for _ in range(k):
            what = rng.random()
            if what < 0.2:
                row.append(None)
            elif what < 0.4:
                row.append(tuple(view))
            else:
                ext = [int(rng.integers(0, v + 1)) for v in view]
                if what < 0.55:
                    ext = list(view)
                    ext[int(rng.integers(rank))] = 0
                row.append(tuple(ext))
        views.append(tuple(view))
        boxes.append(row)
    gaps = [int(rng.choice([0, 1, 2, 9])) for _ in views]
    return build(kind, views, boxes, gaps, seed)


# ------------------------------------------------------------------ 7. the 64-bit path
# Every entry has between 2^30 and 1.01 * 2^30 elements and no extent that is a power of two.  The extents are
# chosen near the upper end: a box cut by one element on every dim loses about n * (1/P + 1/Q + 1/L), and only
# where that is below n - 2^30 do its source indices pass 2^30 at all.  (They cannot for the 4-D view: four
# extents whose reciprocals sum to less than 1 % have a product far above 2^31.)
WIDE_VIEWS = {
    "submodel": [(1040, 1021, 1021), (1061999, 1, 1021)],
    "elastic": [(1, 1, 1, 1084300979), (1, 1, 1061999, 1021), (1, 1040, 1021, 1021), (37, 29, 1009, 997)],
}
WIDE_CUT = (1, 2, 3, 1)      # elements cut from each dim that is not 1, from the last dim backwards, cycling
WIDE_TINY = (7, 5, 3, 2)     # the tiny box's extents, from the last dim that is not 1 backwards
WIDE_RANDOM = 1 << 20
WIDE_EDGE = 2048
WIDE_LEAD = 3                # the entry's offset in g and out
WIDE_SRC = (1, 5, 1)         # client 1 reads client 0's buffer from another src; client 2 has a row of its own


def wide_boxes(view):
    """[cut, half, tiny]: cut by 1-3 elements on every dim that is not 1; about half of the leading dim that
    is not 1 and full elsewhere; at most 3 x 5 x 7 (x 2)."""
    free = [d for d, v in enumerate(view) if v != 1]
    cut, tiny = list(view), [1] * len(view)
    for back, d in enumerate(reversed(free)):
        cut[d] = view[d] - WIDE_CUT[back]
        tiny[d] = WIDE_TINY[back]
    if len(free) == 1:
        tiny[free[0]] = 105
    half = list(view)
    half[free[0]] = view[free[0]] // 2 + 1
    return [tuple(cut), tuple(half), tuple(tiny)]


def wide_row_len(view):
    """The lengths of the three clients' rows: clients 0 and 1 read one buffer."""
    cut, half, tiny = (prod(b) for b in wide_boxes(view))
    shared = max(WIDE_SRC[0] + cut, WIDE_SRC[1] + half) + 1
    return [shared, shared, WIDE_SRC[2] + tiny + 1]


def wide_tables(kind: str, view):
    """(entries, boxes, row_len) of the one-entry call."""
    n = prod(view)
    if kind == "submodel":
        entries = np.array([[WIDE_LEAD, *view, 0, 0]], dtype=np.int64)
        boxes = np.array([[[*b, s] for b, s in zip(wide_boxes(view), WIDE_SRC)]], dtype=np.int64)
    else:
        entries = np.array([[WIDE_LEAD, *view, 0, 0, 3]], dtype=np.int64)
        boxes = np.array([[*b, s, c] for c, (b, s) in enumerate(zip(wide_boxes(view), WIDE_SRC))], dtype=np.int64)
    assert n >= NARROW
    return entries, boxes, np.array(wide_row_len(view), dtype=np.int64)


def wide_tail(view) -> int:
    """The flat index from which the cut box's source indices are at or above 2^30; where the box has fewer
    elements than that, 2^30 itself (the flat indices from there on take more than 30 bits)."""
    cut = wide_boxes(view)[0]
    return flat_of(view, cut, NARROW) if prod(cut) > NARROW else NARROW


def wide_sample(view, seed: int) -> np.ndarray:
    """Sorted flat indices without repeats: 2^20 random ones, half of them over the whole entry and half over
    its tail from `wide_tail` on (under 1 % of an entry lies there: drawn evenly, a sample would hold almost no
    source index above 2^30); the first and last 2,048 elements; 2,048 either side of the end of the half box
    and of flat index 2^30."""
    n = prod(view)
    rng = np.random.default_rng([seed, n])
    half = wide_boxes(view)[1]
    half_end = prod(half)  # full behind its leading dim: its elements are the entry's first prod(half)
    parts = [rng.integers(0, n, size=WIDE_RANDOM // 2), rng.integers(wide_tail(view), n, size=WIDE_RANDOM // 2),
             np.arange(WIDE_EDGE), np.arange(n - WIDE_EDGE, n),
             np.arange(half_end - WIDE_EDGE, half_end + WIDE_EDGE), np.arange(NARROW - WIDE_EDGE, NARROW + WIDE_EDGE)]
    return np.unique(np.concatenate(parts).astype(np.int64))


def wide_cover(view, sample: np.ndarray):
    """[(covered, source index)] per box for the sample, int64."""
    out = []
    for ext in wide_boxes(view):
        c, at = source_index(view, ext, sample)
        c = np.broadcast_to(c, sample.shape)
        out.append((c, np.where(c, at, 0)))
    return out
