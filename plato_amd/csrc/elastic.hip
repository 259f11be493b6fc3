// elastic.hip — gfx950 kernel for the depth- and width-heterogeneous server of the reference's model-search
// examples (examples/model_search/sysheterofl: Algorithm.aggregation), exported through the C ABI in
// include/plato_agg.h as plato_agg_elastic_mean.
//
// Design ("Elastic sub-model aggregation"); the shape is submodel.hip's (§22):
//  * An entry is seen as [A, B, C, D]; a box is (a <= A, b <= B, c <= C, d <= D) of one client and the
//    source of global (i, j, t, u) is row[src + ((i * b + j) * c + t) * d + u].  The box table is compact:
//    an entry names its first box and its number of boxes, and a box names its client, so a tile's loop
//    runs over the clients that hold the entry, not over K.  An entry nobody holds has no boxes.
//  * One launch over all entries.  A workgroup owns one tile of kTile consecutive output elements of one
//    entry: it finds its entry by a binary search of the entries' first tiles (wave-uniform, through the
//    scalar cache), and a lane owns kPer elements kThreads apart, so every load of a wave is a run of 64
//    consecutive dwords of the global region or of one client row.  An element's coordinates cost an
//    integer division only for the view dims whose extent is not 1, the outermost of them excepted (a
//    wave-uniform decision per entry; the host merges the trailing dims that every holder has in full), 32
//    bits wide unless the entry has 2^30 elements or more.  The tile is compiled once per number of view
//    dims from the first that is not 1, so the box loop of a merged convolution ([1, 1, D0, D1 * kh * kw])
//    compares two coordinates and multiplies once.
//  * The box loop runs in table order, sequentially per element: acc = g, then acc = acc + x for the
//    boxes that cover the element, out = (acc - g) / max(count, 1), each fp32 operation separately rounded
//    (the build has -ffp-contract=off).  A box row and its client's row pointer are wave-uniform, read
//    through the scalar cache, the pointer after the box's client word (fetching the next two boxes' rows
//    while the current one is summed took 100 SGPRs and a third more time, and went).  A box whose leading
//    extent ends before the tile is
//    skipped on scalar values, one that covers no lane of the wave by a ballot; otherwise a lane's kPer
//    loads are issued together, the lanes that are not covered reading the box's first element and
//    dropping it.
//  * Nothing in the kernel is sized by K.  No count tensor: the divisor is counted in the loop.
// The tile constants, the entry search, an element's result and the host side's common refusals, entry
// walk and table upload are in boxes.h, shared with submodel.hip; here are the table rows, the coordinates
// per number of view dims, the cover predicate, the box loop with its skips and loads, and the checks of
// the compact box list.
#include "boxes.h"

namespace {

constexpr int kEntryWords = PLATO_AGG_ELASTIC_ENTRY_WORDS;
constexpr int kBoxWords = PLATO_AGG_ELASTIC_BOX_WORDS;
constexpr uint64_t kMaxBoxes = uint64_t(PLATO_AGG_ELASTIC_MAX_ENTRIES) * PLATO_AGG_ELASTIC_MAX_K;

struct Entry {  // one row of the entry table
  int64_t out, A, B, C, D, tile0, box0, n_boxes;
};
struct Box {  // one row of the box table
  int64_t a, b, c, d, src, client;
};
static_assert(sizeof(Entry) == kEntryWords * 8 && sizeof(Box) == kBoxWords * 8, "table rows as the header has them");

// A box row in registers (wave-uniform), its extents narrowed to the index type.
template <class I>
struct BoxRow {
  I a, b, c, d;
  int64_t src, client;
};
template <class I>
__device__ __forceinline__ BoxRow<I> load_box(const int64_t* boxes, uint32_t at) {
  const int64_t* b = boxes + uint64_t(at) * kBoxWords;
  return {I(sld(b, 0)), I(sld(b, 1)), I(sld(b, 2)), I(sld(b, 3)), sld(b, 4), sld(b, 5)};
}

// rem = rem / extent, returning the remainder: the coordinate in a dim of `extent` with `outer` the
// product of the dims before it.  A dim of extent 1 has coordinate 0; the outermost dim that is not 1
// takes what is left without a division.  Both tests are wave-uniform.
template <class I>
__device__ __forceinline__ I peel(I& rem, I extent, I outer) {
  if (extent == 1) return 0;
  I x = rem;
  if (outer == 1) {
    rem = 0;
  } else {
    const I q = rem / extent;
    x = rem - q * extent;
    rem = q;
  }
  return x;
}

// The elements base + threadIdx.x + h * kThreads (h < kPer) of one entry of n elements, viewed [A, B, C, D],
// of which the first 4 - N extents are 1: the box loop compares and multiplies for the last N dims only (a
// merged convolution is N = 2: two compares, one multiplication per element and box).
template <class I, int N>
__device__ __forceinline__ void elastic_tile(const float* __restrict__ g, const float* const* rows,
                                             const int64_t* boxes, uint32_t box0, uint32_t n_boxes,
                                             float* __restrict__ out, I A, I B, I C, I D, uint64_t n,
                                             uint64_t base) {
  I i[kPer], j[kPer], t[kPer], u[kPer];
  bool in[kPer];
  float gv[kPer], acc[kPer];
  uint32_t cnt[kPer];
  const I AB = A * B, ABC = AB * C;  // products of extents: below 2^38, and below 2^30 where I is narrow
#pragma unroll
  for (int h = 0; h < kPer; ++h) {
    const uint64_t f = base + threadIdx.x + uint64_t(h) * kThreads;
    in[h] = f < n;
    const uint64_t at = in[h] ? f : base;  // base < n: a valid element, its value unused
    I rem = I(at);
    u[h] = peel(rem, D, ABC);
    t[h] = peel(rem, C, AB);
    j[h] = peel(rem, B, A);
    i[h] = rem;  // 0 once an inner dim has taken everything
    gv[h] = ((gfloat*)g)[at];
    acc[h] = gv[h];
    cnt[h] = 0;
  }
  if (n_boxes == 0) {  // nobody holds the entry: (g - g) / 1
#pragma unroll
    for (int h = 0; h < kPer; ++h)
      if (in[h]) out[base + threadIdx.x + uint64_t(h) * kThreads] = __fdiv_rn(__fsub_rn(acc[h], gv[h]), 1.0f);
    return;
  }
  // the tile's lowest coordinate in dim 4 - N, the outermost that is not 1 (wave-uniform): that coordinate
  // does not fall inside the tile, so a box whose extent there is at or below it covers nothing here
  const I inner = N == 4 ? B * C * D : N == 3 ? C * D : N == 2 ? D : I(1);
  const I first = I(base) / inner;

  for (uint32_t k = 0; k < n_boxes; ++k) {
    const BoxRow<I> cur = load_box<I>(boxes, box0 + k);
    const float* cur_row = sld(rows, int(cur.client));
    const I ext = N == 4 ? cur.a : N == 3 ? cur.b : N == 2 ? cur.c : cur.d;
    // a box extent in a view dim of 1 is 1, or 0 and the box is empty
    const bool empty = (N < 4 && cur.a == 0) || (N < 3 && cur.b == 0) || (N < 2 && cur.c == 0);
    if (first < ext && !empty) {  // else the whole tile lies past the box
      const float* src = cur_row + cur.src;
      bool c[kPer], any = false;
      I at[kPer];
#pragma unroll
      for (int h = 0; h < kPer; ++h) {
        // `&`, not `&&`: one predicate per element, no branch per lane
        c[h] = in[h] & (u[h] < cur.d);
        I x = 0;
        if (N >= 4) c[h] &= i[h] < cur.a, x = i[h] * cur.b;
        if (N >= 3) c[h] &= j[h] < cur.b, x = (x + j[h]) * cur.c;
        if (N >= 2) c[h] &= t[h] < cur.c, x = (x + t[h]) * cur.d;
        at[h] = c[h] ? x + u[h] : I(0);
        any |= c[h];
      }
      if (__any(any)) {  // else no lane of the wave is covered
        // some lane is covered, so the box has elements and src[0] is one of them: the lanes that are
        // not covered read it and drop it, and the kPer loads are in flight together
        float x[kPer];
#pragma unroll
        for (int h = 0; h < kPer; ++h) x[h] = ((gfloat*)src)[at[h]];
#pragma unroll
        for (int h = 0; h < kPer; ++h) {
          acc[h] = c[h] ? __fadd_rn(acc[h], x[h]) : acc[h];
          cnt[h] += c[h] ? 1u : 0u;
        }
      }
    }
  }
#pragma unroll
  for (int h = 0; h < kPer; ++h)
    if (in[h]) out[base + threadIdx.x + uint64_t(h) * kThreads] = mean_of(acc[h], gv[h], cnt[h]);
}

__global__ __launch_bounds__(kThreads) void elastic_mean_kernel(const float* __restrict__ g,
                                                               const float* const* rows,
                                                               const int64_t* entries, uint32_t n_entries,
                                                               const int64_t* boxes, float* __restrict__ out) {
  const int64_t tile = blockIdx.x;
  const uint32_t lo = find_entry<kEntryWords, 5>(entries, n_entries, tile);
  const int64_t* e = entries + uint64_t(lo) * kEntryWords;  // {out, A, B, C, D, tile0, box0, n_boxes}
  const int64_t off = sld(e, 0);
  const uint64_t A = uint64_t(sld(e, 1)), B = uint64_t(sld(e, 2)), C = uint64_t(sld(e, 3)), D = uint64_t(sld(e, 4));
  const uint64_t n = A * B * C * D;
  const uint64_t base = uint64_t(tile - sld(e, 5)) * kTile;
  const uint32_t box0 = uint32_t(sld(e, 6)), n_boxes = uint32_t(sld(e, 7));
  const int dims = A != 1 ? 4 : B != 1 ? 3 : C != 1 ? 2 : 1;  // wave-uniform, as is the width of the indices
#define ELASTIC_TILE(I, N) \
  elastic_tile<I, N>(g + off, rows, boxes, box0, n_boxes, out + off, I(A), I(B), I(C), I(D), n, base)
  if (n < kNarrow) {
    if (dims == 1) ELASTIC_TILE(uint32_t, 1);
    else if (dims == 2) ELASTIC_TILE(uint32_t, 2);
    else if (dims == 3) ELASTIC_TILE(uint32_t, 3);
    else ELASTIC_TILE(uint32_t, 4);
  } else {
    if (dims == 1) ELASTIC_TILE(uint64_t, 1);
    else if (dims == 2) ELASTIC_TILE(uint64_t, 2);
    else if (dims == 3) ELASTIC_TILE(uint64_t, 3);
    else ELASTIC_TILE(uint64_t, 4);
  }
#undef ELASTIC_TILE
}

}  // namespace

extern "C" {

size_t plato_agg_elastic_tables_bytes(size_t n_entries, size_t n_boxes) {
  if (n_entries > PLATO_AGG_ELASTIC_MAX_ENTRIES || n_boxes > kMaxBoxes) return 0;
  const size_t bytes = round_up(n_entries * sizeof(Entry), 256) + n_boxes * sizeof(Box);
  return bytes ? round_up(bytes, 256) : 256;
}

int plato_agg_elastic_mean(const float* d_global, const float* const* d_rows, int K, const int64_t* h_row_len,
                           const int64_t* h_entries, size_t n_entries, const int64_t* h_boxes, size_t n_boxes,
                           void* d_tables, float* d_out, size_t n_out, hipStream_t stream) {
  const char* why = bad_box_args(d_global, d_rows, K, h_row_len, h_entries, n_entries, h_boxes, n_boxes != 0,
                                 n_boxes > kMaxBoxes ? "more than 2^32 boxes" : nullptr, d_tables, d_out, n_out);
  if (why) return fail(PLATO_AGG_EINVAL, why);
  if (!n_entries || !n_out) return plato_agg_internal::clear_error();

  if (const int bad = check_row_lengths(K, h_row_len)) return bad;
  const Entry* entries = reinterpret_cast<const Entry*>(h_entries);
  const Box* boxes = reinterpret_cast<const Box*>(h_boxes);
  EntryWalk walk;
  uint64_t listed = 0;
  for (size_t e = 0; e < n_entries; ++e) {
    const Entry& en = entries[e];
    const std::string at = "entry " + std::to_string(e);
    why = walk.next(en.out, box_numel({en.A, en.B, en.C, en.D}), en.tile0, 0, n_out);
    if (why) return fail(PLATO_AGG_EINVAL, at + why);
    if (en.box0 < 0 || uint64_t(en.box0) != listed || en.n_boxes < 0 || uint64_t(en.n_boxes) > n_boxes - listed)
      return fail(PLATO_AGG_EINVAL, at + ": box range does not follow the entry before it inside the box table");
    int64_t before = -1;
    for (uint64_t x = listed; x < listed + uint64_t(en.n_boxes); ++x) {
      const Box& b = boxes[x];
      const std::string who = at + ", box " + std::to_string(x - listed);
      if (b.client < 0 || b.client >= K) return fail(PLATO_AGG_EINVAL, who + ": client outside [0, K)");
      if (b.client <= before) return fail(PLATO_AGG_EINVAL, who + ": clients are not strictly ascending");
      before = b.client;
      if (b.a < 0 || b.b < 0 || b.c < 0 || b.d < 0 || b.a > en.A || b.b > en.B || b.c > en.C || b.d > en.D)
        return fail(PLATO_AGG_EINVAL, who + ": box extent above the entry's extent");
      if (past_row(b.src, box_numel({b.a, b.b, b.c, b.d}), h_row_len[b.client]))  // at most the entry's elements
        return fail(PLATO_AGG_EINVAL, who + ": box runs past the client's row length");
    }
    listed += uint64_t(en.n_boxes);
  }
  if (listed != n_boxes) return fail(PLATO_AGG_EINVAL, "the entries' box ranges end before the box table does");
  if (!walk.tiles) return plato_agg_internal::clear_error();  // every entry is empty

  const int64_t* d_boxes;
  if (const int bad = upload_and_check("elastic_mean", d_tables, h_entries, n_entries * sizeof(Entry), h_boxes,
                                       n_boxes * sizeof(Box), stream, &d_boxes))
    return bad;
  hipLaunchKernelGGL(elastic_mean_kernel, dim3(uint32_t(walk.tiles)), dim3(kThreads), 0, stream, d_global, d_rows,
                     static_cast<const int64_t*>(d_tables), uint32_t(n_entries), d_boxes, d_out);
  return launched("elastic_mean");
}

}  // extern "C"
