// rows.h — what robust.hip, krum.hip, trust.hip and detect.hip share: the kernels there all read K client rows through
// a wave-uniform table of row pointers, an fp32 region and an int64 region promoted to fp32, and their
// C-ABI entry points refuse the same malformed arguments with the same words.  Everything is in the
// anonymous namespace, as it was in each of the three files: the kernels' symbols do not change.
// (Not shared: median_kernel / nearest_mean_kernel's load and select, see robust.hip and DESIGN.md §17.)
// submodel.hip and elastic.hip take the table loads and the refusals from here, through boxes.h, which
// holds what only those two share; their rows have lengths of their own.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <initializer_list>
#include <string>

#include "common.h"
#include "plato_agg.h"

namespace {

// ------------------------------------------------------------------ device side
typedef __attribute__((address_space(1))) const float gfloat;
typedef __attribute__((address_space(1))) const int64_t gi64;

// Entry i of a wave-uniform table, through the scalar cache (s_load).
template <class T>
__device__ __forceinline__ T sld(const T* p, int i) {
  return ((__attribute__((address_space(4))) const T*)p)[i];
}

// Coordinate e of one client row as fp32: `load` is the plain load of the streaming and tiled kernels,
// `bits` the nontemporal load of the median kernels (every value is read once and kept in LDS).
template <bool I64>
struct Column;
template <>
struct Column<false> {
  typedef float elem;
  static __device__ __forceinline__ float load(const float* p, uint64_t e) { return ((gfloat*)p)[e]; }
  static __device__ __forceinline__ uint32_t bits(const float* p, uint64_t e) {
    return __float_as_uint(__builtin_nontemporal_load((gfloat*)p + e));
  }
};
template <>
struct Column<true> {
  typedef int64_t elem;
  // torch.cat of fp32 and int64 promotes the counters to fp32, round to nearest even
  static __device__ __forceinline__ float load(const int64_t* p, uint64_t e) { return (float)((gi64*)p)[e]; }
  static __device__ __forceinline__ uint32_t bits(const int64_t* p, uint64_t e) {
    return __float_as_uint((float)__builtin_nontemporal_load((gi64*)p + e));
  }
};

// ------------------------------------------------------------------ host side
inline int fail(int code, const std::string& msg) { return plato_agg_internal::set_error(code, msg); }

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

constexpr uint64_t kMaxCoords = 1ull << 38;  // per region: 2^30 workgroups of 256 in the streaming kernels

// Coordinates per chunk of a region of n coordinates, split for a deterministic reduction: a multiple of
// `unit`, at most `max_chunks` chunks, chosen by n alone.
inline uint64_t chunk_len(uint64_t n, uint64_t unit, uint32_t max_chunks) {
  const uint64_t m = (n + unit * max_chunks - 1) / (unit * max_chunks);
  return unit * (m ? m : 1);
}
inline uint32_t num_chunks(uint64_t n, uint64_t unit, uint32_t max_chunks) {
  const uint64_t len = chunk_len(n, unit, max_chunks);
  return n ? uint32_t((n + len - 1) / len) : 0;
}

// ------------------------------------------------------------------ the fixed-order float64 reduction
// What trust.hip and detect.hip share, so that "the order of plato_agg_trust_stats" is one piece of code:
// the shape of a workgroup (256 lanes, a batch of kU rows, kPer coordinates per lane and pass), the chunking
// of a region by its coordinate count alone, the butterfly over a wave and the final kernel that adds the
// chunks' partials in chunk order.
namespace f64red {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kU = 8;                                 // rows per workgroup
constexpr int kPer = 2;                               // coordinates per lane and pass
constexpr uint64_t kTile = PLATO_AGG_TRUST_TILE;      // a chunk is a whole number of these
constexpr uint64_t kPass = uint64_t(kThreads) * kPer;
constexpr uint32_t kMaxChunks = 1024;                 // coordinate chunks per region, at most
static_assert(kTile % kPass == 0, "a tile is a whole number of passes");

// Coordinates per chunk of a region of n coordinates: a multiple of kTile, chosen by n alone.
inline uint64_t region_chunk_len(uint64_t n) { return chunk_len(n, kTile, kMaxChunks); }
inline uint32_t region_chunks(uint64_t n) { return num_chunks(n, kTile, kMaxChunks); }
inline uint32_t num_batches(int rows) { return uint32_t(rows + kU - 1) / kU; }

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}

// out[row] = sum over the chunks, in chunk order, of the row's partials ws[chunk * nrows + row].  One
// workgroup per row: the partials are fetched by all lanes at once and added by one, so the order costs LDS
// reads, not a chain of memory round trips.  (A template so that only the files that launch it hold it.)
template <int kBlock>
__global__ __launch_bounds__(kBlock) void final_kernel(const double* __restrict__ ws, uint64_t nrows,
                                                      uint32_t nchunks, double* __restrict__ out) {
  __shared__ double part[2 * kMaxChunks];
  const uint64_t row = blockIdx.x;
  for (uint32_t c = threadIdx.x; c < nchunks; c += kBlock) part[c] = ws[uint64_t(c) * nrows + row];
  __syncthreads();
  if (threadIdx.x == 0) {
    double sum = 0.0;
    for (uint32_t c = 0; c < nchunks; ++c) sum += part[c];
    out[row] = sum;
  }
}

}  // namespace f64red

// The refusals of the entry points.  Each returns its message, or nullptr for arguments it accepts; an
// entry point lists its checks in the order it refuses in and reports the first (they only compare their
// arguments, so evaluating all of them costs nothing).
inline const char* first_refusal(std::initializer_list<const char*> checks) {
  for (const char* why : checks)
    if (why) return why;
  return nullptr;
}
inline const char* bad_rows(int K, const char* why) { return K < 1 || K > PLATO_AGG_ROBUST_MAX_K ? why : nullptr; }
// a region with coordinates needs its pointer table and its companion (output or reference vector)
inline const char* null_region(size_t n_f32, const void* x_f32, const void* y_f32, size_t n_i64, const void* x_i64,
                               const void* y_i64) {
  if (n_f32 && (!x_f32 || !y_f32)) return "null fp32 arena pointer";
  if (n_i64 && (!x_i64 || !y_i64)) return "null int64 arena pointer";
  return nullptr;
}
inline const char* bad_tables(size_t n_f32, const void* x_f32, size_t n_i64, const void* x_i64) {
  return (n_f32 && !aligned(x_f32, 8)) || (n_i64 && !aligned(x_i64, 8)) ? "pointer tables must be 8-byte aligned"
                                                                         : nullptr;
}
inline const char* bad_outputs(size_t n_f32, const float* out_f32, size_t n_i64, const float* out_i64_as_f32) {
  return (n_f32 && !aligned(out_f32, 16)) || (n_i64 && !aligned(out_i64_as_f32, 4))
             ? "fp32 output must be 16-byte aligned (int64-as-fp32 output: 4)"
             : nullptr;
}
inline const char* null_f64_out(const double* out, const void* workspace) {
  return !out || !workspace ? "null output or workspace pointer" : nullptr;
}
inline const char* bad_f64_out(const double* out, const char* out_why, const void* workspace) {
  if (!aligned(out, 16)) return out_why;
  return aligned(workspace, 256) ? nullptr : "workspace must be 256-byte aligned";
}
inline const char* too_many_coords(size_t n_f32, size_t n_i64) {
  return n_f32 >= kMaxCoords || n_i64 >= kMaxCoords ? "more than 2^38 coordinates in one call" : nullptr;
}

}  // namespace
