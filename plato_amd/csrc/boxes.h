// boxes.h — what submodel.hip and elastic.hip share: both kernels give a workgroup one tile of one entry,
// found by a binary search of the entry table, and divide what the covering boxes add to the global value
// by their count; and their C-ABI entry points refuse the same malformed arguments with the same words,
// walk the entry table the same way and upload two tables before the launch.  Everything is in the
// anonymous namespace, as it was in each of the two files: the kernels' symbols do not change.
// (Not shared: the table rows, the coordinates of an element, the cover predicates and the box loop with
// its skips and its loads, see each file; the two kernels stay two)
#pragma once

#include "rows.h"

namespace {

// ------------------------------------------------------------------ device side
constexpr int kThreads = 256;
constexpr int kPer = 4;                        // output elements per lane
constexpr uint64_t kTile = uint64_t(kThreads) * kPer;
static_assert(kTile == PLATO_AGG_SUBMODEL_TILE && kTile == PLATO_AGG_ELASTIC_TILE,
              "a tile is one pass of a workgroup");
constexpr uint64_t kNarrow = 1ull << 30;       // entries below this many elements are indexed in 32 bits

// The last entry whose first tile (word kTile0Word of its row of kEntryWords) is at or before `tile`
// (entries without tiles share the first tile of the next entry, which comes later in the table).
// Wave-uniform, through the scalar cache.
template <int kEntryWords, int kTile0Word>
__device__ __forceinline__ uint32_t find_entry(const int64_t* entries, uint32_t n_entries, int64_t tile) {
  uint32_t lo = 0, hi = n_entries - 1;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (sld(entries, int(mid) * kEntryWords + kTile0Word) <= tile)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

// An element's result: (acc - g) / max(count, 1), each operation separately rounded.  The arguments are the
// lane's array elements by reference, read where they are used: that, and the load-and-add block of the box
// loop written out in each kernel, keeps the compiled kernels instruction for instruction what they were
// before this header (as helpers over the lane's arrays they came out with other schedules and, for
// elastic_mean_kernel, one more VGPR).
__device__ __forceinline__ float mean_of(const float& acc, const float& g, const uint32_t& cnt) {
  return __fdiv_rn(__fsub_rn(acc, g), float(cnt ? cnt : 1u));
}

// ------------------------------------------------------------------ host side
static_assert(PLATO_AGG_SUBMODEL_MAX_K == PLATO_AGG_ELASTIC_MAX_K &&
                  PLATO_AGG_SUBMODEL_MAX_ENTRIES == PLATO_AGG_ELASTIC_MAX_ENTRIES,
              "one refusal list for both entry points");

inline size_t round_up(size_t x, size_t m) { return (x + m - 1) / m * m; }

inline bool bad_k(int K) { return K < 1 || K > PLATO_AGG_SUBMODEL_MAX_K; }

// The product of the extents if every factor and the product stay below kMaxCoords, else kMaxCoords
inline uint64_t box_numel(std::initializer_list<int64_t> extents) {
  uint64_t n = 1;
  for (int64_t v : extents) {
    if (v < 0 || uint64_t(v) >= kMaxCoords) return kMaxCoords;
    n *= uint64_t(v);
    if (n >= kMaxCoords) return kMaxCoords;
  }
  return n;
}

// The refusals that only compare the arguments, in the order both entry points refuse in.  `boxes_why` is
// the caller's own refusal of its number of boxes (nullptr where the box table is sized by K), and the box
// table may be null where `need_boxes` is false.
inline const char* bad_box_args(const float* d_global, const float* const* d_rows, int K, const int64_t* h_row_len,
                                const int64_t* h_entries, size_t n_entries, const int64_t* h_boxes,
                                bool need_boxes, const char* boxes_why, const void* d_tables, const float* d_out,
                                size_t n_out) {
  const bool work = n_entries && n_out;
  return first_refusal({
      bad_k(K) ? "K must be in 1..4096" : nullptr,
      n_entries > PLATO_AGG_SUBMODEL_MAX_ENTRIES ? "more than 2^20 entries" : nullptr,
      boxes_why,
      work && (!d_global || !d_out) ? "null fp32 arena pointer" : nullptr,
      work && (!d_rows || !h_row_len) ? "null client row table" : nullptr,
      work && (!h_entries || (need_boxes && !h_boxes) || !d_tables) ? "null entry or box table" : nullptr,
      work && (!aligned(d_rows, 8) || !aligned(h_row_len, 8) || !aligned(h_entries, 8) || !aligned(h_boxes, 8))
          ? "pointer tables must be 8-byte aligned"
          : nullptr,
      work && !aligned(d_tables, 256) ? "the device tables must be 256-byte aligned" : nullptr,
      work && !aligned(d_global, 4) ? "the global region must be 4-byte aligned" : nullptr,
      work ? bad_outputs(n_out, d_out, 0, nullptr) : nullptr,
      too_many_coords(n_out, 0),
  });
}

// 0, or the status of the refusal of the first client whose row length is out of range.
inline int check_row_lengths(int K, const int64_t* h_row_len) {
  for (int k = 0; k < K; ++k)
    if (h_row_len[k] < 0 || uint64_t(h_row_len[k]) >= kMaxCoords)
      return fail(PLATO_AGG_EINVAL, "client " + std::to_string(k) + ": row length outside [0, 2^38)");
  return 0;
}

// The walk over the entry table: where the entries before this one end in the output and in tiles.
struct EntryWalk {
  uint64_t tiles = 0, end = 0;
  // Refuses (with what follows "entry e") or takes the next entry: n elements (box_numel of its view) at
  // `out`, first tile `tile0`, and `reserved` the word that has to be 0 (0 for a table without one).
  const char* next(int64_t out, uint64_t n, int64_t tile0, int64_t reserved, size_t n_out) {
    if (n >= kMaxCoords) return ": bad view extents";
    if (out < 0 || uint64_t(out) < end || uint64_t(out) + n > n_out)
      return ": output range outside the region or overlapping the entry before it";
    if (tile0 < 0 || uint64_t(tile0) != tiles || reserved != 0)
      return ": first tile is not the number of tiles before it";
    end = uint64_t(out) + n;
    tiles += (n + kTile - 1) / kTile;
    return nullptr;
  }
};

// A box of m elements at src of a client row of row_len elements: does it run past the row?
inline bool past_row(int64_t src, uint64_t m, int64_t row_len) {
  return src < 0 || uint64_t(src) > uint64_t(row_len) || m > uint64_t(row_len) - uint64_t(src);
}

// The tables to d_tables, behind the caller's earlier work on the stream (the caller keeps its host tables
// unchanged until the stream has passed the call): the entries, then the boxes at the next multiple of 256
// bytes, which *d_boxes receives.  0, or the status of the failed copy, reported as "<kernel> tables: ...".
inline int upload_and_check(const char* kernel, void* d_tables, const int64_t* h_entries, size_t entry_bytes,
                            const int64_t* h_boxes, size_t box_bytes, hipStream_t stream, const int64_t** d_boxes) {
  char* dev = static_cast<char*>(d_tables);
  *d_boxes = reinterpret_cast<const int64_t*>(dev + round_up(entry_bytes, 256));
  hipError_t err = hipMemcpyAsync(dev, h_entries, entry_bytes, hipMemcpyHostToDevice, stream);
  if (err == hipSuccess && box_bytes)
    err = hipMemcpyAsync(const_cast<int64_t*>(*d_boxes), h_boxes, box_bytes, hipMemcpyHostToDevice, stream);
  if (err != hipSuccess) return fail(PLATO_AGG_EHIP, std::string(kernel) + " tables: " + hipGetErrorString(err));
  return 0;
}

// The status of the call after its launch, a failed one reported as "<kernel>: ...".
inline int launched(const char* kernel) {
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(PLATO_AGG_EHIP, std::string(kernel) + ": " + hipGetErrorString(err));
  return plato_agg_internal::clear_error();
}

}  // namespace
