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
#include "rows.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPer = 4;                        // output elements per lane
constexpr uint64_t kTile = PLATO_AGG_SUBMODEL_TILE;
static_assert(kTile == uint64_t(kThreads) * kPer, "a tile is one pass of a workgroup");
constexpr int kEntryWords = PLATO_AGG_SUBMODEL_ENTRY_WORDS;
constexpr int kBoxWords = PLATO_AGG_SUBMODEL_BOX_WORDS;
constexpr uint64_t kNarrow = 1ull << 30;       // entries below this many elements are indexed in 32 bits

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
    if (in[h])
      out[base + threadIdx.x + uint64_t(h) * kThreads] =
          __fdiv_rn(__fsub_rn(acc[h], gv[h]), float(cnt[h] ? cnt[h] : 1u));
}

__global__ __launch_bounds__(kThreads) void submodel_mean_kernel(const float* __restrict__ g,
                                                                const float* const* rows, int K,
                                                                const int64_t* entries, uint32_t n_entries,
                                                                const int64_t* boxes, float* __restrict__ out) {
  // the last entry whose first tile is at or before this workgroup's (entries without tiles share the
  // first tile of the next entry, which comes later in the table)
  const int64_t tile = blockIdx.x;
  uint32_t lo = 0, hi = n_entries - 1;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (sld(entries, int(mid) * kEntryWords + 4) <= tile)
      lo = mid;
    else
      hi = mid - 1;
  }
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

inline size_t round_up(size_t x, size_t m) { return (x + m - 1) / m * m; }

inline bool bad_k(int K) { return K < 1 || K > PLATO_AGG_SUBMODEL_MAX_K; }

// a * b * c if every factor and the product stay below kMaxCoords, else kMaxCoords
inline uint64_t box_numel(int64_t a, int64_t b, int64_t c) {
  uint64_t n = 1;
  for (int64_t v : {a, b, c}) {
    if (v < 0 || uint64_t(v) >= kMaxCoords) return kMaxCoords;
    n *= uint64_t(v);
    if (n >= kMaxCoords) return kMaxCoords;
  }
  return n;
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
  const bool work = n_entries && n_out;
  const char* why = first_refusal({
      bad_k(K) ? "K must be in 1..4096" : nullptr,
      n_entries > PLATO_AGG_SUBMODEL_MAX_ENTRIES ? "more than 2^20 entries" : nullptr,
      work && (!d_global || !d_out) ? "null fp32 arena pointer" : nullptr,
      work && (!d_rows || !h_row_len) ? "null client row table" : nullptr,
      work && (!h_entries || !h_boxes || !d_tables) ? "null entry or box table" : nullptr,
      work && (!aligned(d_rows, 8) || !aligned(h_row_len, 8) || !aligned(h_entries, 8) || !aligned(h_boxes, 8))
          ? "pointer tables must be 8-byte aligned"
          : nullptr,
      work && !aligned(d_tables, 256) ? "the device tables must be 256-byte aligned" : nullptr,
      work && !aligned(d_global, 4) ? "the global region must be 4-byte aligned" : nullptr,
      work ? bad_outputs(n_out, d_out, 0, nullptr) : nullptr,
      too_many_coords(n_out, 0),
  });
  if (why) return fail(PLATO_AGG_EINVAL, why);
  if (!work) return plato_agg_internal::clear_error();

  for (int k = 0; k < K; ++k)
    if (h_row_len[k] < 0 || uint64_t(h_row_len[k]) >= kMaxCoords)
      return fail(PLATO_AGG_EINVAL, "client " + std::to_string(k) + ": row length outside [0, 2^38)");
  const Entry* entries = reinterpret_cast<const Entry*>(h_entries);
  const Box* boxes = reinterpret_cast<const Box*>(h_boxes);
  uint64_t tiles = 0, end = 0;
  for (size_t e = 0; e < n_entries; ++e) {
    const Entry& en = entries[e];
    const std::string at = "entry " + std::to_string(e);
    const uint64_t n = box_numel(en.P, en.Q, en.L);
    if (n >= kMaxCoords) return fail(PLATO_AGG_EINVAL, at + ": bad view extents");
    if (en.out < 0 || uint64_t(en.out) < end || uint64_t(en.out) + n > n_out)
      return fail(PLATO_AGG_EINVAL, at + ": output range outside the region or overlapping the entry before it");
    if (en.tile0 < 0 || uint64_t(en.tile0) != tiles || en.reserved != 0)
      return fail(PLATO_AGG_EINVAL, at + ": first tile is not the number of tiles before it");
    end = uint64_t(en.out) + n;
    tiles += (n + kTile - 1) / kTile;
    for (int k = 0; k < K; ++k) {
      const Box& b = boxes[e * size_t(K) + k];
      const std::string who = at + ", client " + std::to_string(k);
      if (b.src == PLATO_AGG_SUBMODEL_ABSENT) {
        if (b.p || b.q || b.l) return fail(PLATO_AGG_EINVAL, who + ": an absent box has extents");
        continue;
      }
      if (b.p < 0 || b.q < 0 || b.l < 0 || b.p > en.P || b.q > en.Q || b.l > en.L)
        return fail(PLATO_AGG_EINVAL, who + ": box extent above the global's extent");
      const uint64_t m = box_numel(b.p, b.q, b.l);  // <= n
      if (b.src < 0 || uint64_t(b.src) > uint64_t(h_row_len[k]) || m > uint64_t(h_row_len[k]) - uint64_t(b.src))
        return fail(PLATO_AGG_EINVAL, who + ": box runs past the client's row length");
    }
  }
  if (!tiles) return plato_agg_internal::clear_error();  // every entry is empty

  // the tables, behind the caller's earlier work on the stream; the caller keeps its host tables
  // unchanged until the stream has passed this call
  char* dev = static_cast<char*>(d_tables);
  const size_t entry_bytes = n_entries * sizeof(Entry);
  Box* d_boxes = reinterpret_cast<Box*>(dev + round_up(entry_bytes, 256));
  hipError_t err = hipMemcpyAsync(dev, h_entries, entry_bytes, hipMemcpyHostToDevice, stream);
  if (err == hipSuccess)
    err = hipMemcpyAsync(d_boxes, h_boxes, n_entries * size_t(K) * sizeof(Box), hipMemcpyHostToDevice, stream);
  if (err != hipSuccess) return fail(PLATO_AGG_EHIP, std::string("submodel_mean tables: ") + hipGetErrorString(err));
  hipLaunchKernelGGL(submodel_mean_kernel, dim3(uint32_t(tiles)), dim3(kThreads), 0, stream, d_global, d_rows, K,
                     reinterpret_cast<const int64_t*>(dev), uint32_t(n_entries),
                     reinterpret_cast<const int64_t*>(d_boxes), d_out);
  err = hipGetLastError();
  if (err != hipSuccess) return fail(PLATO_AGG_EHIP, std::string("submodel_mean: ") + hipGetErrorString(err));
  return plato_agg_internal::clear_error();
}

}  // extern "C"
