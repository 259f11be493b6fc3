// attack.hip — gfx950 kernels for the attack simulation of the reference's detector example
// (examples/detector/attacks.py: lie_attack, lambda_attack, min_max_attack, min_sum_attack), exported
// through the C ABI in include/plato_agg.h as plato_agg_column_std and plato_agg_add_scaled_rows.
//
// Design ("Attack simulation"):
//  * column_std is a streaming kernel: a lane owns four consecutive coordinates, read as one 16-byte load
//    per row where the row is 16-byte aligned (the engine's rows are; a wave-uniform test per row picks
//    four 4-byte loads otherwise), through the wave-uniform pointer table.  Per coordinate it runs ATen's
//    sequential float64 Welford update in row order: one subtraction, one IEEE division by the row count
//    so far, one addition, one subtraction, one multiplication, one addition, each separately rounded
//    (the build has -ffp-contract=off).  The rows are taken kRows at a time, every load of a batch issued
//    before its first update; the four coordinates of a lane are four independent chains.  No cross-lane
//    arithmetic: coordinate e depends on column e alone.
//  * add_scaled_rows adds one vector, scaled once, to m distinct rows in place: t = s * v[e] is formed
//    once per coordinate, then a batch of kRows rows is loaded, added to and stored.  The counters take
//    the truncated t, with the x86-64 conversion's results for NaN and out-of-range values.
#include "rows.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPer = 4;    // coordinates per lane: one 16-byte fp32 load per row
constexpr int kRows = 4;   // rows per batch of loads
constexpr uint64_t kTileCoords = uint64_t(kThreads) * kPer;

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Coordinates e0 .. e0 + cnt - 1 of one row as fp32 (cnt <= kPer; the rest are +0 and never stored).
template <bool I64>
__device__ __forceinline__ void load_coords(const typename Column<I64>::elem* p, uint64_t e0, uint32_t cnt,
                                            float (&c)[kPer]) {
  if constexpr (!I64) {
    if (cnt == kPer && aligned16(p)) {  // e0 is a multiple of 4
      const float4 q = *reinterpret_cast<const float4*>(p + e0);
      c[0] = q.x, c[1] = q.y, c[2] = q.z, c[3] = q.w;
      return;
    }
  }
#pragma unroll
  for (uint32_t j = 0; j < kPer; ++j) c[j] = j < cnt ? Column<I64>::load(p, e0 + j) : 0.0f;
}

// ------------------------------------------------------------------ torch.std(X, dim=0), unbiased
template <bool I64>
__global__ __launch_bounds__(kThreads) void column_std_kernel(const typename Column<I64>::elem* const* x, int m,
                                                             float* __restrict__ out, uint64_t n) {
  const uint64_t e0 = (uint64_t(blockIdx.x) * kThreads + threadIdx.x) * kPer;
  if (e0 >= n) return;
  const uint32_t cnt = n - e0 < kPer ? uint32_t(n - e0) : kPer;
  double mean[kPer], m2[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) mean[j] = 0.0, m2[j] = 0.0;
  for (int r0 = 0; r0 < m; r0 += kRows) {
    float c[kRows][kPer];
#pragma unroll
    for (int i = 0; i < kRows; ++i)
      if (r0 + i < m) load_coords<I64>(sld(x, r0 + i), e0, cnt, c[i]);
#pragma unroll
    for (int i = 0; i < kRows; ++i) {
      if (r0 + i >= m) break;
      const double count = double(r0 + i + 1);
#pragma unroll
      for (int j = 0; j < kPer; ++j) {
        const double v = double(c[i][j]);
        const double d = v - mean[j];
        mean[j] = mean[j] + d / count;
        m2[j] = m2[j] + d * (v - mean[j]);
      }
    }
  }
  const double dof = double(m - 1);  // m == 1: 0 / 0 = NaN, as torch
  float s[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) s[j] = float(__dsqrt_rn(m2[j] / dof));
  if (cnt == kPer && aligned16(out)) {
    *reinterpret_cast<float4*>(out + e0) = make_float4(s[0], s[1], s[2], s[3]);
  } else {
#pragma unroll
    for (uint32_t j = 0; j < kPer; ++j)
      if (j < cnt) out[e0 + j] = s[j];
  }
}

// ------------------------------------------------------------------ x_r += s * v, every row r
// plato_agg_cast_f32_i64's conversion: truncation toward zero; NaN and values outside [-2^63, 2^63) give
// INT64_MIN (the x86-64 conversion result of the reference's .long()).
__device__ __forceinline__ int64_t trunc_f32_i64(float f) {
  if (!(f >= -9223372036854775808.0f && f < 9223372036854775808.0f)) return INT64_MIN;
  return (int64_t)f;
}

__global__ __launch_bounds__(kThreads) void add_scaled_f32_kernel(float* const* x, int m, float s,
                                                                 const float* __restrict__ v, uint64_t n) {
  const uint64_t e0 = (uint64_t(blockIdx.x) * kThreads + threadIdx.x) * kPer;
  if (e0 >= n) return;
  const uint32_t cnt = n - e0 < kPer ? uint32_t(n - e0) : kPer;
  float t[kPer];
  load_coords<false>(v, e0, cnt, t);
#pragma unroll
  for (int j = 0; j < kPer; ++j) t[j] = __fmul_rn(s, t[j]);
  for (int r0 = 0; r0 < m; r0 += kRows) {
    // the rows are distinct buffers: a batch's loads all come before its stores
    float* p[kRows];
    float c[kRows][kPer];
#pragma unroll
    for (int i = 0; i < kRows; ++i)
      if (r0 + i < m) {
        p[i] = sld(x, r0 + i);
        load_coords<false>(p[i], e0, cnt, c[i]);
      }
#pragma unroll
    for (int i = 0; i < kRows; ++i) {
      if (r0 + i >= m) break;
#pragma unroll
      for (int j = 0; j < kPer; ++j) c[i][j] = __fadd_rn(c[i][j], t[j]);
      if (cnt == kPer && aligned16(p[i])) {
        *reinterpret_cast<float4*>(p[i] + e0) = make_float4(c[i][0], c[i][1], c[i][2], c[i][3]);
      } else {
#pragma unroll
        for (uint32_t j = 0; j < kPer; ++j)
          if (j < cnt) p[i][e0 + j] = c[i][j];
      }
    }
  }
}

// The counters: one coordinate per lane (a model has a handful of them).  int64 addition wraps, as torch's.
__global__ __launch_bounds__(kThreads) void add_scaled_i64_kernel(int64_t* const* x, int m, float s,
                                                                 const float* __restrict__ v, uint64_t n) {
  const uint64_t e = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (e >= n) return;
  const uint64_t t = uint64_t(trunc_f32_i64(__fmul_rn(s, v[e])));
  for (int r0 = 0; r0 < m; r0 += kRows) {
    int64_t* p[kRows];
    uint64_t c[kRows];
#pragma unroll
    for (int i = 0; i < kRows; ++i)
      if (r0 + i < m) {
        p[i] = sld(x, r0 + i);
        c[i] = uint64_t(p[i][e]);
      }
#pragma unroll
    for (int i = 0; i < kRows; ++i)
      if (r0 + i < m) p[i][e] = int64_t(c[i] + t);
  }
}

uint32_t tiles(size_t n) { return uint32_t((uint64_t(n) + kTileCoords - 1) / kTileCoords); }

int launched(const char* what) {
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(PLATO_AGG_EHIP, std::string(what) + ": " + hipGetErrorString(err));
  return plato_agg_internal::clear_error();
}

}  // namespace

extern "C" {

int plato_agg_column_std(const float* const* d_x_f32, const int64_t* const* d_x_i64, int m, float* d_out_f32,
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
    hipLaunchKernelGGL((column_std_kernel<false>), dim3(tiles(n_f32)), dim3(kThreads), 0, stream, d_x_f32, m,
                       d_out_f32, uint64_t(n_f32));
  if (n_i64)
    hipLaunchKernelGGL((column_std_kernel<true>), dim3(tiles(n_i64)), dim3(kThreads), 0, stream, d_x_i64, m,
                       d_out_i64_as_f32, uint64_t(n_i64));
  return n_f32 || n_i64 ? launched("column_std") : plato_agg_internal::clear_error();
}

int plato_agg_add_scaled_rows(float* const* d_x_f32, int64_t* const* d_x_i64, int m, float s, const float* d_v_f32,
                              const float* d_v_i64_as_f32, size_t n_f32, size_t n_i64, hipStream_t stream) {
  const char* why = first_refusal({
      bad_rows(m, "m must be in 1..256"),
      null_region(n_f32, d_x_f32, d_v_f32, n_i64, d_x_i64, d_v_i64_as_f32),
      bad_tables(n_f32, d_x_f32, n_i64, d_x_i64),
      (n_f32 && !aligned(d_v_f32, 4)) || (n_i64 && !aligned(d_v_i64_as_f32, 4))
          ? "the added vector must be 4-byte aligned"
          : nullptr,
      too_many_coords(n_f32, n_i64),
  });
  if (why) return fail(PLATO_AGG_EINVAL, why);
  if (n_f32)
    hipLaunchKernelGGL(add_scaled_f32_kernel, dim3(tiles(n_f32)), dim3(kThreads), 0, stream, d_x_f32, m, s, d_v_f32,
                       uint64_t(n_f32));
  if (n_i64)
    hipLaunchKernelGGL(add_scaled_i64_kernel, dim3(uint32_t((uint64_t(n_i64) + kThreads - 1) / kThreads)),
                       dim3(kThreads), 0, stream, d_x_i64, m, s, d_v_i64_as_f32, uint64_t(n_i64));
  return n_f32 || n_i64 ? launched("add_scaled_rows") : plato_agg_internal::clear_error();
}

}  // extern "C"
