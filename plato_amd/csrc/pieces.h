// pieces.h — what prune.hip and qsgd_encode.hip share: the walk over the pieces of one fp32 device row.
//
// A piece is an element range [begin, end) of the row (a plato_agg_chunk; `entry` is not read).  The pieces
// of a table are ascending and disjoint; they may be empty and need not start on a 16-byte boundary.  They
// are tiled per piece: tile j of a piece [b, e) is the row's elements [a + j W, a + (j + 1) W) that lie in
// [b, e), with a = b rounded down to 4 elements, so that every 16-byte load of a tile is aligned whatever b
// is.  A tile wholly inside its piece is read with 16-byte loads; the first and last tile of a piece take a
// guarded path that touches nothing outside [b, e).  Tiles are numbered piece after piece: tile order is
// flat-index order.  A workgroup takes the tiles blockIdx.x, blockIdx.x + gridDim.x, ...
//
// Everything is in the anonymous namespace, as rows.h has it: each file holds its own kernels.
#pragma once

#include "rows.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSlots = 4;                                 // 16-byte slots per lane and tile
constexpr uint32_t kTile = PLATO_AGG_PRUNE_TILE;          // W: elements per workgroup and grid step
constexpr uint32_t kGrid = PLATO_AGG_PRUNE_GRID;          // G: workgroups of a streaming launch, at most
static_assert(kTile == uint32_t(kThreads) * kSlots * 4, "a tile is kSlots 16-byte slots per lane");
constexpr uint32_t kMaxPieces = 1u << 20;

typedef __attribute__((address_space(1))) const uint32_t gu32;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const u32x4 gu32x4;

struct Tiles {
  const plato_agg_chunk* pieces;
  const uint32_t* first_tile;  // [n_pieces]: the tiles of the pieces before
  uint32_t n_pieces, n_tiles;
};

__host__ __device__ inline uint32_t tiles_of(uint32_t begin, uint32_t end) {
  return end > begin ? uint32_t((uint64_t(end) - (begin & ~3u) + kTile - 1) / kTile) : 0;
}

// One lane's share of a tile: kSlots groups of 4 consecutive elements, slot s at tile offset 4 * (s * 256 + tid).
struct Share {
  uint64_t at[kSlots];   // row index of the slot's first element
  u32x4 bits[kSlots];
  uint32_t valid[kSlots];  // bit c: element at[s] + c is in the piece
  uint32_t piece;          // the tile's piece (uniform)
  bool full;               // the whole tile is inside its piece (uniform)
};

__device__ __forceinline__ void load_tile(const uint32_t* row, const Tiles& tl, uint32_t t, Share& sh) {
  // the last piece p with first_tile[p] <= t; first_tile[0] = 0 and t < n_tiles (uniform: scalar loads)
  uint32_t lo = 0, hi = tl.n_pieces;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (sld(tl.first_tile, int(mid)) <= t) lo = mid; else hi = mid;
  }
  const uint64_t b = sld(&tl.pieces[lo].begin, 0), e = sld(&tl.pieces[lo].end, 0);
  const uint64_t tb = (b & ~uint64_t(3)) + uint64_t(t - sld(tl.first_tile, int(lo))) * kTile;
  sh.piece = lo;
  sh.full = tb >= b && tb + kTile <= e;
  if (sh.full) {
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
      sh.at[s] = tb + 4 * uint64_t(s * kThreads + threadIdx.x);
      sh.bits[s] = *(gu32x4*)(row + sh.at[s]);
      sh.valid[s] = 0xf;
    }
  } else {
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
      sh.at[s] = tb + 4 * uint64_t(s * kThreads + threadIdx.x);
      sh.valid[s] = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const uint64_t i = sh.at[s] + c;
        const bool in = i >= b && i < e;
        sh.bits[s][c] = in ? ((gu32*)row)[i] : 0u;
        sh.valid[s] |= uint32_t(in) << c;
      }
    }
  }
}

__device__ __forceinline__ uint32_t key_of(uint32_t bits) { return bits & 0x7fffffffu; }

template <class T>
__device__ __forceinline__ T wave_inclusive(T x) {
  const uint32_t lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const T y = __shfl_up(x, off, 64);
    if (lane >= uint32_t(off)) x += y;
  }
  return x;
}

// ------------------------------------------------------------------ a[i] = sum of the entries before i
// One workgroup, 256 entries a step.  kFromPieces: the entries are the tile counts of the pieces (this is
// what fills Tiles::first_tile).  gate: leave at once when *gate is 0.
template <bool kFromPieces>
__global__ __launch_bounds__(kThreads) void scan_kernel(uint32_t* __restrict__ a, uint32_t n,
                                                       const plato_agg_chunk* __restrict__ pieces,
                                                       const uint32_t* __restrict__ gate) {
  if (gate && !*gate) return;
  __shared__ uint32_t wt[2][kWaves];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t carry = 0;
  for (uint32_t i0 = 0, it = 0; i0 < n; i0 += kThreads, ++it) {
    const uint32_t i = i0 + threadIdx.x;
    uint32_t x = 0;
    if (i < n) x = kFromPieces ? tiles_of(pieces[i].begin, pieces[i].end) : a[i];
    const uint32_t incl = wave_inclusive(x);
    if (lane == 63) wt[it & 1][wave] = incl;
    __syncthreads();  // one barrier a step: the next step writes the other buffer
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < kWaves; ++w) {
      const uint32_t v = wt[it & 1][w];
      before += w < wave ? v : 0;
      all += v;
    }
    if (i < n) a[i] = carry + before + incl - x;
    carry += all;
  }
}

// ------------------------------------------------------------------ host side
struct Plan {
  uint64_t n_total = 0;
  uint64_t n_tiles = 0;
};

// The checks of the piece table; fills `plan`.
inline const char* bad_pieces(const plato_agg_chunk* h, size_t n_pieces, size_t n_row, Plan* plan) {
  uint64_t last_end = 0;
  for (size_t p = 0; p < n_pieces; ++p) {
    if (h[p].end < h[p].begin) return "a piece ends before it begins";
    if (h[p].begin < last_end) return "the pieces overlap or are out of order";
    if (h[p].end > n_row) return "a piece ends past the row";
    last_end = h[p].end;
    plan->n_total += h[p].end - h[p].begin;
    plan->n_tiles += tiles_of(h[p].begin, h[p].end);
  }
  return nullptr;
}

constexpr size_t round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

}  // namespace
