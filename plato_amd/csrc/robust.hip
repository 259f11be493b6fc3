// robust.hip — gfx950 kernels for the coordinate-wise median over K client arenas (the "Median"
// aggregator of the reference's examples/detector/aggregations.py) and for the mean of the values
// nearest it (the last step of its "Trimmed-mean" and "Bulyan"), exported through the C ABI in
// include/plato_agg.h as plato_agg_robust_columns.
//
// Design ("Robust aggregation", and §20 for the nearest-mean kernel):
//  * Element-independent like FedAvg: one coordinate per lane, K coalesced dword loads through the
//    wave-uniform pointer table (s_load).
//  * The median is a pure selection, so there is no rounding: the result is bit-exact.  Floats are
//    mapped to order-preserving unsigned keys (sign-flip transform: -0 < +0, -inf / +inf / subnormals
//    are ordinary values); NaNs are tracked beside the selection (the largest |x| bit pattern of the
//    column).
//  * The column lives in LDS as keys[k][lane] (one-wave workgroups, K * 256 bytes, conflict-free:
//    lane l always reads bank l), and its element of rank (K-1)/2 is found by a most-significant-bit
//    first radix select: 32 passes, each counting the keys that agree with the bits fixed so far and
//    have a 0 in the current bit.  Every loop is a run-time loop over K, so one kernel serves every
//    K in 1..256 with a few dozen VGPRs and no scratch.  A lane reads only what it wrote itself: no
//    barrier is needed.
#include "rows.h"

namespace {

// Order-preserving key of an fp32 bit pattern: unsigned ascending = the total order -nan < -inf < ...
// < -0 < +0 < ... < +inf < +nan.
__device__ __forceinline__ uint32_t to_key(uint32_t u) { return u ^ (uint32_t((int32_t)u >> 31) | 0x80000000u); }
__device__ __forceinline__ uint32_t from_key(uint32_t k) { return k ^ (uint32_t((int32_t)~k >> 31) | 0x80000000u); }

constexpr int kWave = 64;  // one-wave workgroups: lane l owns coordinate blockIdx.x * 64 + l

// Lower median of column e over the K rows of `x`.
template <bool I64>
__global__ __launch_bounds__(kWave) void median_kernel(const typename Column<I64>::elem* const* x, int K,
                                                        float* __restrict__ out, uint64_t n) {
  extern __shared__ uint32_t keys[];  // [K][kWave]
  const uint32_t lane = threadIdx.x;
  const uint64_t e = uint64_t(blockIdx.x) * kWave + lane;
  if (e >= n) return;
  uint32_t mag = 0;  // max |x| bit pattern of the column: above +inf's <=> a NaN
#pragma unroll 8
  for (int k = 0; k < K; ++k) {
    const uint32_t u = Column<I64>::bits(sld(x, k), e);
    const uint32_t m = u & 0x7fffffffu;
    mag = mag > m ? mag : m;
    keys[k * kWave + lane] = to_key(u);
  }
  uint32_t rank = uint32_t(K - 1) / 2, sel = 0;
  for (int bit = 31; bit >= 0; --bit) {
    uint32_t below = 0;  // candidates (keys equal to sel above `bit`) with a 0 in `bit`
#pragma unroll 8
    for (int k = 0; k < K; ++k) below += ((keys[k * kWave + lane] ^ sel) >> bit) == 0 ? 1u : 0u;
    if (rank >= below) {
      rank -= below;
      sel |= 1u << bit;
    }
  }
  out[e] = __uint_as_float(mag > 0x7f800000u ? 0x7fc00000u : from_key(sel));
}

// Mean of the K - 2 * trim values of column e nearest its lower median (PLATO_AGG_ROBUST_NEAREST_MEAN).
// The median's load and select, restated here (sharing them through device functions is allowed only
// while median_kernel's ISA stays what DESIGN.md §17 measured), then a second select over the same LDS
// array: keys[k][lane] is overwritten with the bit pattern of |c_k - med|, whose unsigned order is
// 0 < ... < +inf < NaN with bit 31 always clear (31 passes).  Only the set of kept rows matters, not
// their order by distance: the last pass walks the table once, keeps every key below the threshold and
// the first `ties` rows at it, and sums the kept values, reloaded from global memory, in table order.
template <bool I64>
__global__ __launch_bounds__(kWave) void nearest_mean_kernel(const typename Column<I64>::elem* const* x, int K, int trim,
                                                              float* __restrict__ out, uint64_t n) {
  extern __shared__ uint32_t keys[];  // [K][kWave]
  const uint32_t lane = threadIdx.x;
  const uint64_t e = uint64_t(blockIdx.x) * kWave + lane;
  if (e >= n) return;
  uint32_t mag = 0;  // max |x| bit pattern of the column: above +inf's <=> a NaN
#pragma unroll 8
  for (int k = 0; k < K; ++k) {
    const uint32_t u = Column<I64>::bits(sld(x, k), e);
    const uint32_t m = u & 0x7fffffffu;
    mag = mag > m ? mag : m;
    keys[k * kWave + lane] = to_key(u);
  }
  uint32_t rank = uint32_t(K - 1) / 2, sel = 0;
  for (int bit = 31; bit >= 0; --bit) {
    uint32_t below = 0;
#pragma unroll 8
    for (int k = 0; k < K; ++k) below += ((keys[k * kWave + lane] ^ sel) >> bit) == 0 ? 1u : 0u;
    if (rank >= below) {
      rank -= below;
      sel |= 1u << bit;
    }
  }
  const float med = __uint_as_float(from_key(sel));
#pragma unroll 8
  for (int k = 0; k < K; ++k) {
    const float c = __uint_as_float(from_key(keys[k * kWave + lane]));
    const uint32_t d = __float_as_uint(c - med) & 0x7fffffffu;  // one rounded subtraction, sign cleared
    keys[k * kWave + lane] = d > 0x7f800000u ? 0x7fc00000u : d;  // inf - inf: after +inf
  }
  const uint32_t kept = uint32_t(K - 2 * trim);
  rank = kept - 1, sel = 0;
  for (int bit = 30; bit >= 0; --bit) {
    uint32_t below = 0;
#pragma unroll 8
    for (int k = 0; k < K; ++k) below += ((keys[k * kWave + lane] ^ sel) >> bit) == 0 ? 1u : 0u;
    if (rank >= below) {
      rank -= below;
      sel |= 1u << bit;
    }
  }
  // sel is the key of rank kept - 1, and rank is now its position among the keys equal to it
  uint32_t ties = rank + 1;
  float acc = 0.0f;
#pragma unroll 8
  for (int k = 0; k < K; ++k) {
    const uint32_t d = keys[k * kWave + lane];
    const float c = __uint_as_float(Column<I64>::bits(sld(x, k), e));
    const bool tie = d == sel && ties != 0;  // lowest table position first
    ties -= tie ? 1u : 0u;
    acc = (d < sel || tie) ? acc + c : acc;
  }
  out[e] = mag > 0x7f800000u ? __uint_as_float(0x7fc00000u) : acc / float(kept);
}

template <bool I64>
void launch_median(const void* x, int K, float* out, size_t n, hipStream_t st) {
  hipLaunchKernelGGL((median_kernel<I64>), dim3(uint32_t((n + kWave - 1) / kWave)), dim3(kWave),
                     size_t(K) * kWave * sizeof(uint32_t), st, (const typename Column<I64>::elem* const*)x, K, out,
                     uint64_t(n));
}

template <bool I64>
void launch_nearest_mean(const void* x, int K, int trim, float* out, size_t n, hipStream_t st) {
  hipLaunchKernelGGL((nearest_mean_kernel<I64>), dim3(uint32_t((n + kWave - 1) / kWave)), dim3(kWave),
                     size_t(K) * kWave * sizeof(uint32_t), st, (const typename Column<I64>::elem* const*)x, K, trim,
                     out, uint64_t(n));
}

}  // namespace

extern "C" {

int plato_agg_robust_columns(int mode, const float* const* d_x_f32, const int64_t* const* d_x_i64, int K, int trim,
                             float* d_out_f32, float* d_out_i64_as_f32, size_t n_f32, size_t n_i64,
                             hipStream_t stream) {
  const char* why = first_refusal({
      bad_rows(K, "K must be in 1..256"),
      mode != PLATO_AGG_ROBUST_MEDIAN && mode != PLATO_AGG_ROBUST_NEAREST_MEAN ? "unknown robust aggregation mode"
                                                                               : nullptr,
      trim < 0 || 2 * trim >= K ? "trim must satisfy 0 <= 2*trim < K" : nullptr,
      null_region(n_f32, d_x_f32, d_out_f32, n_i64, d_x_i64, d_out_i64_as_f32),
      bad_tables(n_f32, d_x_f32, n_i64, d_x_i64),
      bad_outputs(n_f32, d_out_f32, n_i64, d_out_i64_as_f32),
      // one coordinate per lane, at least 64 lanes per workgroup, at most 2^31 - 1 workgroups
      n_f32 / 64 >= 0x7fffffffull || n_i64 / 64 >= 0x7fffffffull ? "more than 2^37 coordinates in one call" : nullptr,
  });
  if (why) return fail(PLATO_AGG_EINVAL, why);
  if (mode == PLATO_AGG_ROBUST_MEDIAN) {
    if (n_f32) launch_median<false>(d_x_f32, K, d_out_f32, n_f32, stream);
    if (n_i64) launch_median<true>(d_x_i64, K, d_out_i64_as_f32, n_i64, stream);
  } else {
    if (n_f32) launch_nearest_mean<false>(d_x_f32, K, trim, d_out_f32, n_f32, stream);
    if (n_i64) launch_nearest_mean<true>(d_x_i64, K, trim, d_out_i64_as_f32, n_i64, stream);
  }
  if (n_f32 || n_i64) {
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(PLATO_AGG_EHIP, std::string("robust_columns: ") + hipGetErrorString(err));
  }
  return plato_agg_internal::clear_error();
}

}  // extern "C"
