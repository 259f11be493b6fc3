// krum.hip — gfx950 kernels for the distance-based aggregators of the reference's detector example
// (examples/detector/aggregations.py: multi_krum), exported through the C ABI in include/plato_agg.h as
// plato_agg_pairwise_sqdist and plato_agg_mean_rows.
//
// Design ("Multi-Krum"):
//  * pairwise_sqdist is the one kernel here that HBM does not bound: at K = 128 every loaded float
//    takes part in ~64 pair updates (one v_sub_f32 and one v_fma_f32 each), so it is tiled for the
//    vector ALU.  The lane is the coordinate.  A wave keeps an 8 x 8 block of pair accumulators in
//    VGPRs; a 16-wave workgroup covers a 32 x 32 client tile and stages a panel of (32 + 32 client
//    rows) x 128 coordinates in LDS, double buffered: the next panel's global loads are in flight
//    while the current one is consumed, one barrier per panel.  A row is fetched once per 32 x 32
//    tile; only tiles on or above the diagonal are computed (the lower triangle is its mirror), and
//    a diagonal tile computes its 10 upper 8 x 8 blocks only.
//  * Arithmetic: d = fp32(c_i[e] - c_j[e]), acc = fma(d, d, acc) in fp32 chains of at most
//    PLATO_AGG_PAIRDIST_CHAIN terms per lane.  A finished chain is widened to float64 and the 64 lanes
//    are summed by a fixed butterfly (lane ^ 32, ^ 16, ... ^ 1, a reduce-scatter: lane l ends with
//    the sum of accumulator l); that sum is added to a per-lane float64 total.  Every workgroup covers
//    one fixed coordinate chunk (a function of the coordinate count alone) and writes its totals to
//    the workspace; a final kernel adds the chunks in chunk order.  No atomics: the result is
//    repeatable, and out[i][j] depends on rows i and j and on (n_f32, n_i64) only.  (a - b)^2 and
//    (b - a)^2 have the same bits, so the matrix is symmetric bitwise.
//  * mean_rows is a streaming kernel in the shape of the FedAvg one: one coordinate per lane, m
//    coalesced loads through the wave-uniform pointer table, sequential fp32 adds, one IEEE division.
#include "rows.h"

namespace {

// ------------------------------------------------------------------ pairwise squared distances
constexpr int kTile = 32;                     // clients per tile side
constexpr int kBlock = 8;                     // clients per wave block side
constexpr int kWaves = 16;                    // (kTile / kBlock)^2
constexpr int kThreads = kWaves * 64;
constexpr int kPanel = 128;                   // coordinates per LDS panel: two per lane
constexpr int kRows = 2 * kTile;              // panel rows: the i tile, then the j tile
constexpr int kLoads = kRows * kPanel / kThreads;  // dwords a thread stages per panel (8)
constexpr int kChain = PLATO_AGG_PAIRDIST_CHAIN;
constexpr int kChainPanels = kChain * 64 / kPanel;  // panels per fp32 chain
constexpr uint64_t kChainCoords = uint64_t(kChain) * 64;
constexpr uint32_t kMaxChunks = 256;          // coordinate chunks per region, at most
static_assert(kChain % 2 == 0 && kChainPanels >= 1, "a chain covers whole panels");
static_assert(kLoads * kThreads == kRows * kPanel, "the panel divides among the threads");

// Coordinates per chunk of a region of n coordinates: a multiple of the chain's 64 * kChain, chosen by n alone.
uint64_t chunk_len(uint64_t n) { return chunk_len(n, kChainCoords, kMaxChunks); }
uint32_t num_chunks(uint64_t n) { return num_chunks(n, kChainCoords, kMaxChunks); }
uint32_t num_tiles(int K) {
  const uint32_t t = uint32_t(K + kTile - 1) / kTile;
  return t * (t + 1) / 2;
}

// The 8 x 8 blocks (bi <= bj) of a diagonal tile, one per wave 0..9; waves 10..15 only stage.
__constant__ const uint8_t kDiagBi[10] = {0, 0, 0, 0, 1, 1, 1, 2, 2, 3};
__constant__ const uint8_t kDiagBj[10] = {0, 1, 2, 3, 1, 2, 3, 2, 3, 3};

// Sum over the 64 lanes of each of the 64 fp32 accumulators, in float64, by a fixed butterfly: lane l
// returns the sum of acc[l].  Level by level a lane keeps the half of its values whose index has the
// level's bit equal to its own lane bit and hands the other half to lane ^ bit.  IEEE addition is
// commutative, so both partners form the same bits.
__device__ __forceinline__ double lane_sums(const float (&acc)[64], uint32_t lane) {
  double s32[32];
  {
    const bool hi = lane & 32;
#pragma unroll
    for (int a = 0; a < 32; ++a) {
      const float keep = hi ? acc[a + 32] : acc[a];
      const float send = hi ? acc[a] : acc[a + 32];
      s32[a] = double(keep) + double(__shfl_xor(send, 32));
    }
  }
  double s16[16], s8[8], s4[4], s2[2];
#define PLATO_LEVEL(dst, src, n, bit)                               \
  {                                                                 \
    const bool hi = lane & (bit);                                   \
    _Pragma("unroll") for (int a = 0; a < (n); ++a) {               \
      const double keep = hi ? src[a + (n)] : src[a];               \
      const double send = hi ? src[a] : src[a + (n)];               \
      dst[a] = keep + __shfl_xor(send, (bit));                      \
    }                                                               \
  }
  PLATO_LEVEL(s16, s32, 16, 16)
  PLATO_LEVEL(s8, s16, 8, 8)
  PLATO_LEVEL(s4, s8, 4, 4)
  PLATO_LEVEL(s2, s4, 2, 2)
#undef PLATO_LEVEL
  const bool hi = lane & 1;
  const double keep = hi ? s2[1] : s2[0];
  const double send = hi ? s2[0] : s2[1];
  return keep + __shfl_xor(send, 1);
}

// One workgroup: client tile `tile` (upper triangle, row-major enumeration) x coordinate chunk `chunk`
// of one region.  ws[((chunk0 + chunk) * ntiles + tile) * 1024 + li * 32 + lj] = the chunk's partial of
// pair (ti * 32 + li, tj * 32 + lj); entries of blocks that are not computed are never read.
template <bool I64>
__global__ __launch_bounds__(kThreads) void pairdist_kernel(const typename Column<I64>::elem* const* x, int K,
                                                           uint64_t n, uint64_t clen, uint32_t ntiles,
                                                           uint32_t chunk0, double* __restrict__ ws) {
  __shared__ float panel[2][kRows * kPanel];  // 64 KiB
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t tile = blockIdx.x % ntiles, chunk = blockIdx.x / ntiles;
  // tile -> (ti <= tj)
  const uint32_t T = uint32_t(K + kTile - 1) / kTile;
  uint32_t ti = 0, rest = tile;
  while (rest >= T - ti) {
    rest -= T - ti;
    ++ti;
  }
  const uint32_t tj = ti + rest;
  const bool diag = ti == tj;
  // this wave's block of the tile
  uint32_t bi = wave >> 2, bj = wave & 3;
  bool active = true;
  if (diag) {
    active = wave < 10;
    bi = kDiagBi[active ? wave : 0];
    bj = kDiagBj[active ? wave : 0];
  }
  // the rows this wave stages: panel rows wave * 4 + q, clamped to the last client (tile padding is
  // computed on a copy of a valid row and never read back)
  const typename Column<I64>::elem* rows[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint32_t r = wave * 4 + q;
    uint32_t c = (r < kTile ? ti * kTile + r : tj * kTile + r - kTile);
    c = c < uint32_t(K) ? c : uint32_t(K) - 1;
    rows[q] = sld(x, int(c));
  }
  const uint64_t begin = uint64_t(chunk) * clen;
  const uint64_t end = begin + clen < n ? begin + clen : n;
  const uint32_t npanels = uint32_t((end - begin + kPanel - 1) / kPanel);

  float stage[kLoads];
  auto fetch = [&](uint32_t p) {
    const uint64_t e0 = begin + uint64_t(p) * kPanel + lane;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const uint64_t e = e0 + h * 64;
        stage[q * 2 + h] = e < end ? Column<I64>::load(rows[q], e) : 0.0f;  // 0 - 0 adds nothing to a chain
      }
  };
  auto store = [&](uint32_t buf) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int h = 0; h < 2; ++h) panel[buf][(wave * 4 + q) * kPanel + h * 64 + lane] = stage[q * 2 + h];
  };

  float acc[64];
#pragma unroll
  for (int a = 0; a < 64; ++a) acc[a] = 0.0f;
  double total = 0.0;

  fetch(0);
  store(0);
  __syncthreads();
  for (uint32_t p = 0; p < npanels; ++p) {
    const uint32_t buf = p & 1;
    if (p + 1 < npanels) fetch(p + 1);
    if (active) {
      const float* pa = &panel[buf][(bi * kBlock) * kPanel + lane];
      const float* pb = &panel[buf][(kTile + bj * kBlock) * kPanel + lane];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        float a[kBlock], b[kBlock];
#pragma unroll
        for (int r = 0; r < kBlock; ++r) {
          a[r] = pa[r * kPanel + h * 64];
          b[r] = pb[r * kPanel + h * 64];
        }
#pragma unroll
        for (int r = 0; r < kBlock; ++r)
#pragma unroll
          for (int c = 0; c < kBlock; ++c) {
            const float d = __fsub_rn(a[r], b[c]);
            acc[r * kBlock + c] = __fmaf_rn(d, d, acc[r * kBlock + c]);
          }
      }
      if ((p + 1) % kChainPanels == 0 || p + 1 == npanels) {  // the chain is full, or the chunk ends
        total += lane_sums(acc, lane);
#pragma unroll
        for (int a = 0; a < 64; ++a) acc[a] = 0.0f;
      }
    }
    // buf ^ 1 was last read before the previous barrier
    if (p + 1 < npanels) store(buf ^ 1);
    __syncthreads();
  }
  if (active) {
    const uint32_t li = bi * kBlock + (lane >> 3), lj = bj * kBlock + (lane & 7);
    ws[(uint64_t(chunk0 + chunk) * ntiles + tile) * (kTile * kTile) + li * kTile + lj] = total;
  }
}

// out[i][j] = sum over the chunks, in chunk order, of the pair's partials; the diagonal is +0.
__global__ __launch_bounds__(256) void pairdist_final_kernel(const double* __restrict__ ws, int K, uint32_t nchunks,
                                                            uint32_t ntiles, double* __restrict__ out) {
  const uint32_t idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= uint32_t(K) * uint32_t(K)) return;
  const uint32_t i = idx / uint32_t(K), j = idx % uint32_t(K);
  if (i == j) {
    out[idx] = 0.0;
    return;
  }
  const uint32_t a = i < j ? i : j, b = i < j ? j : i;
  const uint32_t T = uint32_t(K + kTile - 1) / kTile;
  const uint32_t ti = a / kTile, tj = b / kTile;
  const uint32_t tile = ti * T - ti * (ti - 1) / 2 + (tj - ti);
  const uint64_t at = uint64_t(tile) * (kTile * kTile) + (a % kTile) * kTile + (b % kTile);
  double sum = 0.0;
  for (uint32_t c = 0; c < nchunks; ++c) sum += ws[uint64_t(c) * ntiles * (kTile * kTile) + at];
  out[idx] = sum;
}

// ------------------------------------------------------------------ mean of m rows
template <bool I64>
__global__ __launch_bounds__(256) void mean_rows_kernel(const typename Column<I64>::elem* const* x, int m,
                                                       float* __restrict__ out, uint64_t n) {
  const uint64_t e = uint64_t(blockIdx.x) * 256 + threadIdx.x;
  if (e >= n) return;
  float acc = 0.0f;
#pragma unroll 8
  for (int r = 0; r < m; ++r) acc = __fadd_rn(acc, Column<I64>::load(sld(x, r), e));
  out[e] = __fdiv_rn(acc, (float)m);
}

}  // namespace

extern "C" {

size_t plato_agg_pairwise_sqdist_workspace(int K, size_t n_f32, size_t n_i64) {
  if (K < 1 || K > PLATO_AGG_ROBUST_MAX_K || n_f32 >= kMaxCoords || n_i64 >= kMaxCoords) return 0;
  const size_t chunks = size_t(num_chunks(n_f32)) + num_chunks(n_i64);
  const size_t bytes = chunks * num_tiles(K) * (kTile * kTile) * sizeof(double);
  return bytes ? bytes : 256;
}

int plato_agg_pairwise_sqdist(const float* const* d_x_f32, const int64_t* const* d_x_i64, int K, size_t n_f32,
                              size_t n_i64, void* d_workspace, double* d_out, hipStream_t stream) {
  const char* why = first_refusal({
      bad_rows(K, "K must be in 1..256"),
      null_region(n_f32, d_x_f32, d_x_f32, n_i64, d_x_i64, d_x_i64),
      null_f64_out(d_out, d_workspace),
      bad_tables(n_f32, d_x_f32, n_i64, d_x_i64),
      bad_f64_out(d_out, "the distance matrix must be 16-byte aligned", d_workspace),
      too_many_coords(n_f32, n_i64),
  });
  if (why) return fail(PLATO_AGG_EINVAL, why);
  const uint32_t ntiles = num_tiles(K), cf = num_chunks(n_f32), ci = num_chunks(n_i64);
  double* ws = static_cast<double*>(d_workspace);
  if (cf)
    hipLaunchKernelGGL((pairdist_kernel<false>), dim3(cf * ntiles), dim3(kThreads), 0, stream, d_x_f32, K,
                       uint64_t(n_f32), chunk_len(n_f32), ntiles, 0u, ws);
  if (ci)
    hipLaunchKernelGGL((pairdist_kernel<true>), dim3(ci * ntiles), dim3(kThreads), 0, stream, d_x_i64, K,
                       uint64_t(n_i64), chunk_len(n_i64), ntiles, cf, ws);
  hipLaunchKernelGGL(pairdist_final_kernel, dim3((uint32_t(K) * uint32_t(K) + 255) / 256), dim3(256), 0, stream, ws, K,
                     cf + ci, ntiles, d_out);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(PLATO_AGG_EHIP, std::string("pairwise_sqdist: ") + hipGetErrorString(err));
  return plato_agg_internal::clear_error();
}

int plato_agg_mean_rows(const float* const* d_x_f32, const int64_t* const* d_x_i64, int m, float* d_out_f32,
                        float* d_out_i64_as_f32, size_t n_f32, size_t n_i64, hipStream_t stream) {
  const char* why = first_refusal({
      bad_rows(m, "m must be in 1..256"),
      null_region(n_f32, d_x_f32, d_out_f32, n_i64, d_x_i64, d_out_i64_as_f32),
      bad_tables(n_f32, d_x_f32, n_i64, d_x_i64),
      bad_outputs(n_f32, d_out_f32, n_i64, d_out_i64_as_f32),
      too_many_coords(n_f32, n_i64),
  });
  if (why) return fail(PLATO_AGG_EINVAL, why);
  if (n_f32)
    hipLaunchKernelGGL((mean_rows_kernel<false>), dim3(uint32_t((n_f32 + 255) / 256)), dim3(256), 0, stream, d_x_f32,
                       m, d_out_f32, uint64_t(n_f32));
  if (n_i64)
    hipLaunchKernelGGL((mean_rows_kernel<true>), dim3(uint32_t((n_i64 + 255) / 256)), dim3(256), 0, stream, d_x_i64,
                       m, d_out_i64_as_f32, uint64_t(n_i64));
  if (n_f32 || n_i64) {
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(PLATO_AGG_EHIP, std::string("mean_rows: ") + hipGetErrorString(err));
  }
  return plato_agg_internal::clear_error();
}

}  // extern "C"
