// submodel.hip — gfx950 kernel for the width-heterogeneous servers of the reference's model-search
// examples (examples/model_search/{heterofl,fjord,fedrolex,anycostfl}: Algorithm.aggregation), exported
// through the C ABI in include/plato_agg.h as plato_agg_submodel_mean.
//
// Design ("Sub-model aggregation"):
//  * Every client holds a leading-corner box of every participating global tensor, packed in a compact
//    row of its own.  An entry is seen as [P, Q, L]; client k's box is (p <= P, q <= Q, l <= L) and the
//    source of global (i, j, t) is row_k[src + (i * q + j) * l + t].
//  * One launch over all entries.  A workgroup owns one tile of kTile consecutive output elements of one
//    entry: it finds its entry by a binary search of the entries' first tiles (wave-uniform, through the
//    scalar cache), and a lane owns kPer elements kThreads apart, so every load of a wave is a run of 64
//    consecutive dwords of the global region or of one client row.  An element's (i, j, t) come from one
//    integer division by L (and one by Q for the rank-3 view), 32 bits wide unless the entry has 2^30
//    elements or more.
//  * The client loop runs in table order, sequentially per element: acc = g, then acc = acc + x_k for the
//    clients that cover the element, out = (acc - g) / max(count, 1), each fp32 operation separately
//    rounded (the build has -ffp-contract=off).  The boxes and the row pointers are wave-uniform tables
//    read through the scalar cache; client reads are dword loads (a client row is unaligned in general).
//    A client whose rows end before the tile is skipped on scalar values, one that covers no lane of the
//    wave by a ballot; otherwise a lane's kPer loads are issued together, the lanes that are not covered
//    reading the box's first element and dropping it.
//  * Nothing in the kernel is sized by K.  No count tensor: the divisor is counted in the loop.
// The tile constants, the entry search, an element's result and the host side's common refusals, entry
// walk and table upload are in boxes.h, shared with elastic.hip; here are the table rows, the coordinates,
// the cover predicate, the client loop with its skips and loads, and the checks of a box.
#include "boxes.h"

namespace {

constexpr int kEntryWords = PLATO_AGG_SUBMODEL_ENTRY_WORDS;
constexpr int kBoxWords = PLATO_AGG_SUBMODEL_BOX_WORDS;

struct Entry {  // one row of the entry table
  int64_t out, P, Q, L, tile0, reserved;
};
struct Box {  // one row of the box table
  int64_t p, q, l, src;
};
static_assert(sizeof(Entry) == kEntryWords * 8 && sizeof(Box) == kBoxWords * 8, "table rows as the header has them");

// The elements base + threadIdx.x + h * kThreads (h < kPer) of one entry of n elements, viewed [P, Q, L].
template <class I>
__device__ __forceinline__ void submodel_tile(const float* __restrict__ g, const float* const* rows, int K,
                                              const int64_t* boxes, float* __restrict__ out, I Q, I L,
                                              uint64_t n, uint64_t base) {
  I i[kPer], j[kPer], t[kPer];
  bool in[kPer];
  float gv[kPer], acc[kPer];
  uint32_t cnt[kPer];
#pragma unroll
  for (int h = 0; h < kPer; ++h) {
    const uint64_t f = base + threadIdx.x + uint64_t(h) * kThreads;
    in[h] = f < n;
    const uint64_t at = in[h] ? f : base;  // base < n: a valid element, its value unused
    const I fi = I(at);
    const I r = fi / L;
    t[h] = fi - r * L;
    if (Q == 1) {
      i[h] = r;
      j[h] = 0;
    } else {
      i[h] = r / Q;
      j[h] = r - i[h] * Q;
    }
    gv[h] = ((gfloat*)g)[at];
    acc[h] = gv[h];
    cnt[h] = 0;
  }
  const I i_first = I(base) / L / Q;  // the tile's lowest first index (wave-uniform)
  for (int k = 0; k < K; ++k) {
    const int64_t* b = boxes + k * kBoxWords;  // {p, q, l, src}; an absent box has no extents
    const I p = I(sld(b, 0)), q = I(sld(b, 1)), l = I(sld(b, 2));
    const float* src = sld(rows, k) + sld(b, 3);
    if (i_first >= p) continue;  // the whole tile lies past the client's rows
    bool c[kPer], any = false;
    I at[kPer];
#pragma unroll
    for (int h = 0; h < kPer; ++h) {
      c[h] = in[h] && i[h] < p && j[h] < q && t[h] < l;
      at[h] = c[h] ? (i[h] * q + j[h]) * l + t[h] : I(0);
      any |= c[h];
    }
    if (!__any(any)) continue;  // no lane of the wave is covered
    // some lane is covered, so the box has elements and src[0] is one of them: the lanes that are not
    // covered read it and drop it, and the kPer loads are in flight together
    float x[kPer];
#pragma unroll
    for (int h = 0; h < kPer; ++h) x[h] = ((gfloat*)src)[at[h]];
#pragma unroll
    for (int h = 0; h < kPer; ++h) {
      acc[h] = c[h] ? __fadd_rn(acc[h], x[h]) : acc[h];
      cnt[h] += c[h] ? 1u : 0u;
    }
  }
#pragma unroll
  for (int h = 0; h < kPer; ++h)
    if (in[h]) out[base + threadIdx.x + uint64_t(h) * kThreads] = mean_of(acc[h], gv[h], cnt[h]);
}

__global__ __launch_bounds__(kThreads) void submodel_mean_kernel(const float* __restrict__ g,
                                                                const float* const* rows, int K,
                                                                const int64_t* entries, uint32_t n_entries,
                                                                const int64_t* boxes, float* __restrict__ out) {
  const int64_t tile = blockIdx.x;
  const uint32_t lo = find_entry<kEntryWords, 4>(entries, n_entries, tile);
  const int64_t* e = entries + uint64_t(lo) * kEntryWords;  // {out, P, Q, L, tile0, 0}
  const int64_t off = sld(e, 0);
  const uint64_t P = uint64_t(sld(e, 1)), Q = uint64_t(sld(e, 2)), L = uint64_t(sld(e, 3));
  const uint64_t n = P * Q * L;
  const uint64_t base = uint64_t(tile - sld(e, 4)) * kTile;
  const int64_t* mine = boxes + uint64_t(lo) * uint32_t(K) * kBoxWords;
  if (n < kNarrow)
    submodel_tile<uint32_t>(g + off, rows, K, mine, out + off, uint32_t(Q), uint32_t(L), n, base);
  else
    submodel_tile<uint64_t>(g + off, rows, K, mine, out + off, Q, L, n, base);
}

}  // namespace

extern "C" {

size_t plato_agg_submodel_tables_bytes(int K, size_t n_entries) {
  if (bad_k(K) || n_entries > PLATO_AGG_SUBMODEL_MAX_ENTRIES) return 0;
  const size_t bytes = round_up(n_entries * sizeof(Entry), 256) + n_entries * size_t(K) * sizeof(Box);
  return bytes ? round_up(bytes, 256) : 256;
}

int plato_agg_submodel_mean(const float* d_global, const float* const* d_rows, int K, const int64_t* h_row_len,
                            const int64_t* h_entries, const int64_t* h_boxes, size_t n_entries, void* d_tables,
                            float* d_out, size_t n_out, hipStream_t stream) {
  const char* why = bad_box_args(d_global, d_rows, K, h_row_len, h_entries, n_entries, h_boxes, true, nullptr,
                                 d_tables, d_out, n_out);
  if (why) return fail(PLATO_AGG_EINVAL, why);
  if (!n_entries || !n_out) return plato_agg_internal::clear_error();

  if (const int bad = check_row_lengths(K, h_row_len)) return bad;
  const Entry* entries = reinterpret_cast<const Entry*>(h_entries);
  const Box* boxes = reinterpret_cast<const Box*>(h_boxes);
  EntryWalk walk;
  for (size_t e = 0; e < n_entries; ++e) {
    const Entry& en = entries[e];
    const std::string at = "entry " + std::to_string(e);
    why = walk.next(en.out, box_numel({en.P, en.Q, en.L}), en.tile0, en.reserved, n_out);
    if (why) return fail(PLATO_AGG_EINVAL, at + why);
    for (int k = 0; k < K; ++k) {
      const Box& b = boxes[e * size_t(K) + k];
      const std::string who = at + ", client " + std::to_string(k);
      if (b.src == PLATO_AGG_SUBMODEL_ABSENT) {
        if (b.p || b.q || b.l) return fail(PLATO_AGG_EINVAL, who + ": an absent box has extents");
        continue;
      }
      if (b.p < 0 || b.q < 0 || b.l < 0 || b.p > en.P || b.q > en.Q || b.l > en.L)
        return fail(PLATO_AGG_EINVAL, who + ": box extent above the global's extent");
      if (past_row(b.src, box_numel({b.p, b.q, b.l}), h_row_len[k]))  // the box has at most the entry's elements
        return fail(PLATO_AGG_EINVAL, who + ": box runs past the client's row length");
    }
  }
  if (!walk.tiles) return plato_agg_internal::clear_error();  // every entry is empty

  const int64_t* d_boxes;
  if (const int bad = upload_and_check("submodel_mean", d_tables, h_entries, n_entries * sizeof(Entry), h_boxes,
                                       n_entries * size_t(K) * sizeof(Box), stream, &d_boxes))
    return bad;
  hipLaunchKernelGGL(submodel_mean_kernel, dim3(uint32_t(walk.tiles)), dim3(kThreads), 0, stream, d_global, d_rows,
                     K, static_cast<const int64_t*>(d_tables), uint32_t(n_entries), d_boxes, d_out);
  return launched("submodel_mean");
}

}  // extern "C"
