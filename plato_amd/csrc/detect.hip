// detect.hip — gfx950 kernels for the FLDetector defence of the reference's detector example
// (examples/detector/detectors.py: fl_detector, lbfgs), exported through the C ABI in include/plato_agg.h as
// plato_agg_detect_means, plato_agg_rows_dots, plato_agg_lbfgs_predict and plato_agg_delta_sqdist.
//
// Design ("FLDetector"):
//  * A flat row is D = n_f32 + n_i64 contiguous fp32 values in arena order: the fp32 region, then the int64
//    region promoted to fp32.  The detector's record, its means and its prediction are flat rows; the client
//    rows and the baseline stay arenas and are read through rows.h's Column<I64>.
//  * detect_means and lbfgs_predict are streaming kernels in the shape of mean_rows: one coordinate per
//    lane, the rows through a wave-uniform pointer table, float64 arithmetic with every operation separately
//    rounded (the build has -ffp-contract=off), one rounding to fp32 at the end.
//  * rows_dots and delta_sqdist are trust_stats' reduction: a workgroup owns one coordinate chunk (its length
//    a function of the coordinate count alone) and one batch of kU rows, the lane is the coordinate, every
//    term is formed in float64 and added per lane in coordinate order, the 64 lanes by a fixed butterfly,
//    the 4 waves through LDS in wave order, the chunks through a workspace by a final kernel in chunk order.
//    No atomics.  rows_dots reads each row once for all of its m vectors; the vectors are re-read once per
//    batch of kU rows by adjacent workgroups, out of the L2.
#include "rows.h"

namespace {

using namespace f64red;  // rows.h: the workgroup shape, the chunking, wave_sum and the final kernel
constexpr int kMaxVecs = PLATO_AGG_DETECT_MAX_VECTORS;

// Client k's delta at coordinate e as plato_agg_compute_deltas forms it, promoted to fp32.
template <bool I64>
struct Delta;
template <>
struct Delta<false> {
  static __device__ __forceinline__ float of(float x, float b) { return __fsub_rn(x, b); }
  static __device__ __forceinline__ float base(const float* b, uint64_t e) { return ((gfloat*)b)[e]; }
};
template <>
struct Delta<true> {
  static __device__ __forceinline__ float of(int64_t x, int64_t b) {
    return (float)(int64_t)((uint64_t)x - (uint64_t)b);  // the wrapping int64 difference, one rounding
  }
  static __device__ __forceinline__ int64_t base(const int64_t* b, uint64_t e) { return ((gi64*)b)[e]; }
};
template <bool I64>
__device__ __forceinline__ typename Column<I64>::elem raw(const typename Column<I64>::elem* p, uint64_t e) {
  typedef __attribute__((address_space(1))) const typename Column<I64>::elem gelem;
  return ((gelem*)p)[e];
}

// ------------------------------------------------------------------ the four means
// g, v, s_new, y_new and the baseline as fp32 of one region; every flat-row pointer is at the region's first
// coordinate.
template <bool I64>
__global__ __launch_bounds__(256) void detect_means_kernel(const typename Column<I64>::elem* const* x, int K,
                                                          const typename Column<I64>::elem* __restrict__ b,
                                                          const float* __restrict__ lw, const float* __restrict__ lg,
                                                          float* __restrict__ g_out, float* __restrict__ v_out,
                                                          float* __restrict__ s_out, float* __restrict__ y_out,
                                                          float* __restrict__ bf_out, uint64_t n) {
  const uint64_t e = uint64_t(blockIdx.x) * 256 + threadIdx.x;
  if (e >= n) return;
  const auto be = Delta<I64>::base(b, e);
  const float w = ((gfloat*)lw)[e];
  double sd = 0.0, sv = 0.0;
#pragma unroll 8
  for (int k = 0; k < K; ++k) {
    const auto xe = raw<I64>(sld(x, k), e);
    sd += (double)Delta<I64>::of(xe, be);
    sv += (double)__fsub_rn((float)xe, w);
  }
  const float g = (float)(sd / (double)K);
  g_out[e] = g;
  v_out[e] = (float)(sv / (double)K);
  s_out[e] = __fsub_rn((float)be, w);
  y_out[e] = __fsub_rn(g, ((gfloat*)lg)[e]);
  bf_out[e] = (float)be;
}

// ------------------------------------------------------------------ dots of flat rows with M vectors
// One workgroup: row batch blockIdx.x x chunk blockIdx.y.  ws[chunk * (R * M) + r * M + j] = the chunk's
// partial of row r with vector j.
template <int M>
__global__ __launch_bounds__(kThreads) void rows_dots_kernel(const float* const* rows_tab, int R,
                                                            const float* const* vecs_tab, uint64_t n, uint64_t clen,
                                                            double* __restrict__ ws) {
  __shared__ double red[kWaves][kU * M];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t chunk = blockIdx.y;
  const uint64_t begin = uint64_t(chunk) * clen;
  const uint64_t end = begin + clen < n ? begin + clen : n;
  double* out = ws + uint64_t(chunk) * (uint64_t(R) * M);

  const int r0 = int(blockIdx.x) * kU;
  // rows past R are a copy of the last row's: computed, never written
  const float* rows[kU];
  const float* vecs[M];
#pragma unroll
  for (int u = 0; u < kU; ++u) rows[u] = sld(rows_tab, r0 + u < R ? r0 + u : R - 1);
#pragma unroll
  for (int j = 0; j < M; ++j) vecs[j] = sld(vecs_tab, j);

  double acc[kU][M];
#pragma unroll
  for (int u = 0; u < kU; ++u)
#pragma unroll
    for (int j = 0; j < M; ++j) acc[u][j] = 0.0;

  for (uint64_t e0 = begin + threadIdx.x; e0 < end; e0 += kPass) {
    float v[M][kPer], c[kU][kPer];
    bool in[kPer];
#pragma unroll
    for (int h = 0; h < kPer; ++h) {
      const uint64_t e = e0 + uint64_t(h) * kThreads;
      in[h] = e < end;
      const uint64_t at = in[h] ? e : e0;  // e0 < end: a valid coordinate, its value unused
#pragma unroll
      for (int j = 0; j < M; ++j) v[j][h] = ((gfloat*)vecs[j])[at];
#pragma unroll
      for (int u = 0; u < kU; ++u) c[u][h] = ((gfloat*)rows[u])[at];
    }
#pragma unroll
    for (int h = 0; h < kPer; ++h) {
      if (!in[h]) continue;
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const double cd = (double)c[u][h];
#pragma unroll
        for (int j = 0; j < M; ++j) acc[u][j] += cd * (double)v[j][h];
      }
    }
  }
#pragma unroll
  for (int u = 0; u < kU; ++u)
#pragma unroll
    for (int j = 0; j < M; ++j) {
      const double t = wave_sum(acc[u][j]);
      if (lane == 0) red[wave][u * M + j] = t;
    }
  __syncthreads();
  if (threadIdx.x < kU * M) {
    const int i = threadIdx.x, u = i / M;
    if (r0 + u < R) {
      double t = 0.0;
      for (int w = 0; w < kWaves; ++w) t += red[w][i];
      out[uint64_t(r0) * M + i] = t;
    }
  }
}

// ------------------------------------------------------------------ squared distances of the deltas to pred
// One workgroup: client batch blockIdx.x x chunk blockIdx.y of one region.
// ws[(chunk0 + chunk) * K + k] = the chunk's partial of client k.
template <bool I64>
__global__ __launch_bounds__(kThreads) void delta_sqdist_kernel(const typename Column<I64>::elem* const* x, int K,
                                                               const typename Column<I64>::elem* __restrict__ b,
                                                               const float* __restrict__ pred, uint64_t n,
                                                               uint64_t clen, uint32_t chunk0,
                                                               double* __restrict__ ws) {
  __shared__ double red[kWaves][kU];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t chunk = blockIdx.y;
  const uint64_t begin = uint64_t(chunk) * clen;
  const uint64_t end = begin + clen < n ? begin + clen : n;
  double* out = ws + uint64_t(chunk0 + chunk) * uint32_t(K);

  const int k0 = int(blockIdx.x) * kU;
  // rows past K are a copy of the last client's: computed, never written
  const typename Column<I64>::elem* rows[kU];
#pragma unroll
  for (int u = 0; u < kU; ++u) rows[u] = sld(x, k0 + u < K ? k0 + u : K - 1);

  double acc[kU];
#pragma unroll
  for (int u = 0; u < kU; ++u) acc[u] = 0.0;

  for (uint64_t e0 = begin + threadIdx.x; e0 < end; e0 += kPass) {
    float p[kPer], d[kU][kPer];
    bool in[kPer];
#pragma unroll
    for (int h = 0; h < kPer; ++h) {
      const uint64_t e = e0 + uint64_t(h) * kThreads;
      in[h] = e < end;
      const uint64_t at = in[h] ? e : e0;  // e0 < end: a valid coordinate, its value unused
      p[h] = ((gfloat*)pred)[at];
      const auto be = Delta<I64>::base(b, at);
#pragma unroll
      for (int u = 0; u < kU; ++u) d[u][h] = Delta<I64>::of(raw<I64>(rows[u], at), be);
    }
#pragma unroll
    for (int h = 0; h < kPer; ++h) {
      if (!in[h]) continue;
      const double pd = (double)p[h];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const double t = pd - (double)d[u][h];
        acc[u] += t * t;
      }
    }
  }
#pragma unroll
  for (int u = 0; u < kU; ++u) {
    const double t = wave_sum(acc[u]);
    if (lane == 0) red[wave][u] = t;
  }
  __syncthreads();
  if (threadIdx.x < kU && k0 + int(threadIdx.x) < K) {
    double t = 0.0;
    for (int w = 0; w < kWaves; ++w) t += red[w][threadIdx.x];
    out[k0 + threadIdx.x] = t;
  }
}

// ------------------------------------------------------------------ the L-BFGS prediction
__global__ __launch_bounds__(256) void lbfgs_predict_kernel(const float* const* rows, int R,
                                                           const double* __restrict__ a, double sigma,
                                                           const float* __restrict__ lg, const float* __restrict__ v,
                                                           float* __restrict__ pred, uint64_t n) {
  const uint64_t e = uint64_t(blockIdx.x) * 256 + threadIdx.x;
  if (e >= n) return;
  double acc = 0.0;
#pragma unroll 8
  for (int j = 0; j < R; ++j) acc += sld(a, j) * (double)((gfloat*)sld(rows, j))[e];
  const double t = (double)((gfloat*)lg)[e] + sigma * (double)((gfloat*)v)[e];
  pred[e] = (float)(t - acc);
}

const char* bad_flat(const void* p) { return !aligned(p, 4) ? "flat rows must be 4-byte aligned" : nullptr; }
const char* bad_base(size_t n_f32, const void* b_f32, size_t n_i64, const void* b_i64) {
  return (n_f32 && !aligned(b_f32, 4)) || (n_i64 && !aligned(b_i64, 8)) ? "the baseline must be 4-byte aligned (int64: 8)"
                                                                         : nullptr;
}
const char* bad_record(int R) {
  return R < 1 || R > PLATO_AGG_DETECT_MAX_ROWS ? "R must be in 1..65536" : nullptr;
}

}  // namespace

extern "C" {

int plato_agg_detect_means(const float* const* d_x_f32, const int64_t* const* d_x_i64, int K, const float* d_b_f32,
                           const int64_t* d_b_i64, const float* d_last_w, const float* d_last_g, float* d_g,
                           float* d_v, float* d_s_new, float* d_y_new, float* d_b_flat, size_t n_f32, size_t n_i64,
                           hipStream_t stream) {
  const bool any = n_f32 || n_i64;
  const char* why = first_refusal({
      bad_rows(K, "K must be in 1..256"),
      null_region(n_f32, d_x_f32, d_b_f32, n_i64, d_x_i64, d_b_i64),
      any && (!d_last_w || !d_last_g || !d_g || !d_v || !d_s_new || !d_y_new || !d_b_flat) ? "null flat row pointer"
                                                                                          : nullptr,
      bad_tables(n_f32, d_x_f32, n_i64, d_x_i64),
      bad_base(n_f32, d_b_f32, n_i64, d_b_i64),
      bad_flat(d_last_w), bad_flat(d_last_g), bad_flat(d_g), bad_flat(d_v), bad_flat(d_s_new), bad_flat(d_y_new),
      bad_flat(d_b_flat),
      too_many_coords(n_f32, n_i64),
  });
  if (why) return fail(PLATO_AGG_EINVAL, why);
  if (!any) return plato_agg_internal::clear_error();
  if (n_f32)
    hipLaunchKernelGGL((detect_means_kernel<false>), dim3(uint32_t((n_f32 + 255) / 256)), dim3(256), 0, stream, d_x_f32,
                       K, d_b_f32, d_last_w, d_last_g, d_g, d_v, d_s_new, d_y_new, d_b_flat, uint64_t(n_f32));
  if (n_i64)
    hipLaunchKernelGGL((detect_means_kernel<true>), dim3(uint32_t((n_i64 + 255) / 256)), dim3(256), 0, stream, d_x_i64,
                       K, d_b_i64, d_last_w + n_f32, d_last_g + n_f32, d_g + n_f32, d_v + n_f32, d_s_new + n_f32,
                       d_y_new + n_f32, d_b_flat + n_f32, uint64_t(n_i64));
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(PLATO_AGG_EHIP, std::string("detect_means: ") + hipGetErrorString(err));
  return plato_agg_internal::clear_error();
}

size_t plato_agg_rows_dots_workspace(int R, int m, size_t D) {
  if (bad_record(R) || m < 1 || m > kMaxVecs || D >= kMaxCoords) return 0;
  const size_t bytes = size_t(region_chunks(D)) * size_t(R) * size_t(m) * sizeof(double);
  return bytes ? bytes : 256;
}

int plato_agg_rows_dots(const float* const* d_rows, int R, const float* const* d_vecs, int m, size_t D,
                        void* d_workspace, double* d_out, hipStream_t stream) {
  const char* why = first_refusal({
      bad_record(R),
      m < 1 || m > kMaxVecs ? "m must be in 1..4" : nullptr,
      D && (!d_rows || !d_vecs) ? "null pointer table" : nullptr,
      null_f64_out(d_out, d_workspace),
      !aligned(d_rows, 8) || !aligned(d_vecs, 8) ? "pointer tables must be 8-byte aligned" : nullptr,
      bad_f64_out(d_out, "the dots must be 16-byte aligned", d_workspace),
      too_many_coords(D, 0),
  });
  if (why) return fail(PLATO_AGG_EINVAL, why);
  if (!D) return plato_agg_internal::clear_error();
  const uint32_t nc = region_chunks(D);
  const dim3 grid(num_batches(R), nc);
  double* ws = static_cast<double*>(d_workspace);
  const uint64_t n = D, clen = region_chunk_len(D);
  switch (m) {
    case 1: hipLaunchKernelGGL((rows_dots_kernel<1>), grid, dim3(kThreads), 0, stream, d_rows, R, d_vecs, n, clen, ws); break;
    case 2: hipLaunchKernelGGL((rows_dots_kernel<2>), grid, dim3(kThreads), 0, stream, d_rows, R, d_vecs, n, clen, ws); break;
    case 3: hipLaunchKernelGGL((rows_dots_kernel<3>), grid, dim3(kThreads), 0, stream, d_rows, R, d_vecs, n, clen, ws); break;
    default: hipLaunchKernelGGL((rows_dots_kernel<4>), grid, dim3(kThreads), 0, stream, d_rows, R, d_vecs, n, clen, ws); break;
  }
  const uint64_t nrows = uint64_t(R) * uint64_t(m);
  hipLaunchKernelGGL(final_kernel<256>, dim3(uint32_t(nrows)), dim3(256), 0, stream, ws, nrows, nc, d_out);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(PLATO_AGG_EHIP, std::string("rows_dots: ") + hipGetErrorString(err));
  return plato_agg_internal::clear_error();
}

int plato_agg_lbfgs_predict(const float* const* d_rows, int R, const double* d_a, double sigma, const float* d_last_g,
                            const float* d_v, float* d_pred, size_t D, hipStream_t stream) {
  const char* why = first_refusal({
      bad_record(R),
      D && (!d_rows || !d_a) ? "null pointer table" : nullptr,
      D && (!d_last_g || !d_v || !d_pred) ? "null flat row pointer" : nullptr,
      !aligned(d_rows, 8) || !aligned(d_a, 8) ? "pointer tables must be 8-byte aligned" : nullptr,
      bad_flat(d_last_g), bad_flat(d_v), bad_flat(d_pred),
      too_many_coords(D, 0),
  });
  if (why) return fail(PLATO_AGG_EINVAL, why);
  if (!D) return plato_agg_internal::clear_error();
  hipLaunchKernelGGL(lbfgs_predict_kernel, dim3(uint32_t((D + 255) / 256)), dim3(256), 0, stream, d_rows, R, d_a, sigma,
                     d_last_g, d_v, d_pred, uint64_t(D));
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(PLATO_AGG_EHIP, std::string("lbfgs_predict: ") + hipGetErrorString(err));
  return plato_agg_internal::clear_error();
}

size_t plato_agg_delta_sqdist_workspace(int K, size_t n_f32, size_t n_i64) {
  if (K < 1 || K > PLATO_AGG_ROBUST_MAX_K || n_f32 >= kMaxCoords || n_i64 >= kMaxCoords) return 0;
  const size_t bytes = (size_t(region_chunks(n_f32)) + region_chunks(n_i64)) * size_t(K) * sizeof(double);
  return bytes ? bytes : 256;
}

int plato_agg_delta_sqdist(const float* const* d_x_f32, const int64_t* const* d_x_i64, int K, const float* d_b_f32,
                           const int64_t* d_b_i64, const float* d_pred, size_t n_f32, size_t n_i64, void* d_workspace,
                           double* d_out, hipStream_t stream) {
  const bool any = n_f32 || n_i64;
  const char* why = first_refusal({
      bad_rows(K, "K must be in 1..256"),
      null_region(n_f32, d_x_f32, d_b_f32, n_i64, d_x_i64, d_b_i64),
      any && !d_pred ? "null flat row pointer" : nullptr,
      null_f64_out(d_out, d_workspace),
      bad_tables(n_f32, d_x_f32, n_i64, d_x_i64),
      bad_base(n_f32, d_b_f32, n_i64, d_b_i64),
      bad_flat(d_pred),
      bad_f64_out(d_out, "the distances must be 16-byte aligned", d_workspace),
      too_many_coords(n_f32, n_i64),
  });
  if (why) return fail(PLATO_AGG_EINVAL, why);
  if (!any) return plato_agg_internal::clear_error();
  const uint32_t cf = region_chunks(n_f32), ci = region_chunks(n_i64), nb = num_batches(K);
  double* ws = static_cast<double*>(d_workspace);
  if (cf)
    hipLaunchKernelGGL((delta_sqdist_kernel<false>), dim3(nb, cf), dim3(kThreads), 0, stream, d_x_f32, K, d_b_f32, d_pred,
                       uint64_t(n_f32), region_chunk_len(n_f32), 0u, ws);
  if (ci)
    hipLaunchKernelGGL((delta_sqdist_kernel<true>), dim3(nb, ci), dim3(kThreads), 0, stream, d_x_i64, K, d_b_i64,
                       d_pred + n_f32, uint64_t(n_i64), region_chunk_len(n_i64), cf, ws);
  hipLaunchKernelGGL(final_kernel<256>, dim3(uint32_t(K)), dim3(256), 0, stream, ws, uint64_t(K), cf + ci, d_out);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(PLATO_AGG_EHIP, std::string("delta_sqdist: ") + hipGetErrorString(err));
  return plato_agg_internal::clear_error();
}

}  // extern "C"
