// trust.hip — gfx950 kernels for the cosine-trust aggregator of the reference's detector example
// (examples/detector/aggregations.py: fl_trust), exported through the C ABI in include/plato_agg.h as
// plato_agg_trust_stats and plato_agg_scaled_sum.
//
// Design ("Fl-trust"):
//  * trust_stats is a streaming reduction: per client the dot product with a reference vector r, the
//    squared norm and the squared norm of fp32(c + eps), plus |r|^2.  A workgroup owns one coordinate
//    chunk (its length a function of the region's coordinate count alone) and one batch of kU clients.
//    The lane is the coordinate: every pass over kPer * 256 coordinates issues kPer coalesced loads of r
//    and kU * kPer of the clients through the wave-uniform pointer table.  Every product is formed in
//    float64 from its fp32 operands (exact) and added to a per-lane float64 accumulator in coordinate
//    order; the 64 lanes are summed by a fixed butterfly, the 4 waves through LDS in wave order, and the
//    workgroup writes one partial per (chunk, value) to the workspace.  A final kernel (one workgroup per
//    value: the partials fetched by all lanes, added by one) adds the chunks in chunk order.  No atomics: the result is repeatable, and client k's three values depend on row k, on
//    r and on (n_f32, n_i64) only — not on K, on the batch the client falls in or on the table order.
//    r is read once per batch of kU clients; the batches of one chunk are adjacent workgroups, so the
//    re-reads are served by the L2.
//  * scaled_sum is a streaming kernel in the shape of mean_rows: one coordinate per lane, K coalesced
//    loads, per row one fp32 multiply, one IEEE division, one multiply and one add, each separately
//    rounded (the build has -ffp-contract=off).
#include "rows.h"

namespace {

// ------------------------------------------------------------------ per-client dots and norms
using namespace f64red;  // rows.h: the workgroup shape, the chunking, wave_sum and the final kernel

// One workgroup: client batch blockIdx.x (batch num_batches(K) is the reference vector's own) x chunk
// blockIdx.y of one region.  ws[(chunk0 + chunk) * (3K + 1) + row] = the chunk's partial of output `row`.
template <bool I64>
__global__ __launch_bounds__(kThreads) void trust_stats_kernel(const typename Column<I64>::elem* const* x, int K,
                                                              const float* __restrict__ ref, float eps, uint64_t n,
                                                              uint64_t clen, uint32_t chunk0,
                                                              double* __restrict__ ws) {
  __shared__ double red[kWaves][3 * kU];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t batch = blockIdx.x, chunk = blockIdx.y;
  const uint32_t nrows = 3 * uint32_t(K) + 1;
  const uint64_t begin = uint64_t(chunk) * clen;
  const uint64_t end = begin + clen < n ? begin + clen : n;
  double* out = ws + uint64_t(chunk0 + chunk) * nrows;

  if (batch == gridDim.x - 1) {  // |r|^2
    double s = 0.0;
    for (uint64_t e = begin + threadIdx.x; e < end; e += kThreads) {
      const double r = (double)((gfloat*)ref)[e];
      s += r * r;
    }
    s = wave_sum(s);
    if (lane == 0) red[wave][0] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = 0.0;
      for (int w = 0; w < kWaves; ++w) t += red[w][0];
      out[3 * uint32_t(K)] = t;
    }
    return;
  }

  const int k0 = int(batch) * kU;
  // rows past K are a copy of the last client's: computed, never written
  const typename Column<I64>::elem* rows[kU];
#pragma unroll
  for (int u = 0; u < kU; ++u) rows[u] = sld(x, k0 + u < K ? k0 + u : K - 1);

  double dot[kU], sq[kU], sqe[kU];
#pragma unroll
  for (int u = 0; u < kU; ++u) dot[u] = sq[u] = sqe[u] = 0.0;

  for (uint64_t e0 = begin + threadIdx.x; e0 < end; e0 += kPass) {
    float r[kPer], c[kU][kPer];
    bool in[kPer];
#pragma unroll
    for (int h = 0; h < kPer; ++h) {
      const uint64_t e = e0 + uint64_t(h) * kThreads;
      in[h] = e < end;
      const uint64_t at = in[h] ? e : e0;  // e0 < end: a valid coordinate, its value unused
      r[h] = ((gfloat*)ref)[at];
#pragma unroll
      for (int u = 0; u < kU; ++u) c[u][h] = Column<I64>::load(rows[u], at);
    }
#pragma unroll
    for (int h = 0; h < kPer; ++h) {
      if (!in[h]) continue;
      const double rd = (double)r[h];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const double cd = (double)c[u][h];
        const double ce = (double)__fadd_rn(c[u][h], eps);
        dot[u] += cd * rd;
        sq[u] += cd * cd;
        sqe[u] += ce * ce;
      }
    }
  }
#pragma unroll
  for (int u = 0; u < kU; ++u) {
    dot[u] = wave_sum(dot[u]);
    sq[u] = wave_sum(sq[u]);
    sqe[u] = wave_sum(sqe[u]);
  }
  if (lane == 0) {
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      red[wave][u] = dot[u];
      red[wave][kU + u] = sq[u];
      red[wave][2 * kU + u] = sqe[u];
    }
  }
  __syncthreads();
  if (threadIdx.x < 3 * kU) {
    const int j = threadIdx.x, u = j % kU, which = j / kU;
    if (k0 + u < K) {
      double t = 0.0;
      for (int w = 0; w < kWaves; ++w) t += red[w][j];
      out[uint32_t(which) * uint32_t(K) + uint32_t(k0 + u)] = t;
    }
  }
}

// ------------------------------------------------------------------ sum of scaled rows
template <bool I64>
__global__ __launch_bounds__(256) void scaled_sum_kernel(const typename Column<I64>::elem* const* x, int K,
                                                        const float* mul, const float* div, float post,
                                                        float* __restrict__ out, uint64_t n) {
  const uint64_t e = uint64_t(blockIdx.x) * 256 + threadIdx.x;
  if (e >= n) return;
  float acc = 0.0f;
#pragma unroll 8
  for (int k = 0; k < K; ++k) {
    float t = __fmul_rn(Column<I64>::load(sld(x, k), e), sld(mul, k));
    t = __fdiv_rn(t, sld(div, k));
    t = __fmul_rn(t, post);
    acc = __fadd_rn(acc, t);
  }
  out[e] = acc;
}

}  // namespace

extern "C" {

size_t plato_agg_trust_stats_workspace(int K, size_t n_f32, size_t n_i64) {
  if (K < 1 || K > PLATO_AGG_ROBUST_MAX_K || n_f32 >= kMaxCoords || n_i64 >= kMaxCoords) return 0;
  const size_t chunks = size_t(region_chunks(n_f32)) + region_chunks(n_i64);
  const size_t bytes = chunks * (3 * size_t(K) + 1) * sizeof(double);
  return bytes ? bytes : 256;
}

int plato_agg_trust_stats(const float* const* d_x_f32, const int64_t* const* d_x_i64, int K, const float* d_ref_f32,
                          const float* d_ref_i64_as_f32, float eps, size_t n_f32, size_t n_i64, void* d_workspace,
                          double* d_out, hipStream_t stream) {
  const char* why = first_refusal({
      bad_rows(K, "K must be in 1..256"),
      null_region(n_f32, d_x_f32, d_ref_f32, n_i64, d_x_i64, d_ref_i64_as_f32),
      null_f64_out(d_out, d_workspace),
      bad_tables(n_f32, d_x_f32, n_i64, d_x_i64),
      (n_f32 && !aligned(d_ref_f32, 4)) || (n_i64 && !aligned(d_ref_i64_as_f32, 4))
          ? "the reference vector must be 4-byte aligned"
          : nullptr,
      bad_f64_out(d_out, "the statistics must be 16-byte aligned", d_workspace),
      too_many_coords(n_f32, n_i64),
  });
  if (why) return fail(PLATO_AGG_EINVAL, why);
  if (!n_f32 && !n_i64) return plato_agg_internal::clear_error();
  const uint32_t cf = region_chunks(n_f32), ci = region_chunks(n_i64), nb = num_batches(K) + 1;
  const uint32_t nrows = 3 * uint32_t(K) + 1;
  double* ws = static_cast<double*>(d_workspace);
  if (cf)
    hipLaunchKernelGGL((trust_stats_kernel<false>), dim3(nb, cf), dim3(kThreads), 0, stream, d_x_f32, K, d_ref_f32, eps,
                       uint64_t(n_f32), region_chunk_len(n_f32), 0u, ws);
  if (ci)
    hipLaunchKernelGGL((trust_stats_kernel<true>), dim3(nb, ci), dim3(kThreads), 0, stream, d_x_i64, K,
                       d_ref_i64_as_f32, eps, uint64_t(n_i64), region_chunk_len(n_i64), cf, ws);
  hipLaunchKernelGGL(final_kernel<256>, dim3(nrows), dim3(256), 0, stream, ws, nrows, cf + ci, d_out);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(PLATO_AGG_EHIP, std::string("trust_stats: ") + hipGetErrorString(err));
  return plato_agg_internal::clear_error();
}

int plato_agg_scaled_sum(const float* const* d_x_f32, const int64_t* const* d_x_i64, int K, const float* d_mul,
                         const float* d_div, float post, float* d_out_f32, float* d_out_i64_as_f32, size_t n_f32,
                         size_t n_i64, hipStream_t stream) {
  const char* why = first_refusal({
      bad_rows(K, "K must be in 1..256"),
      null_region(n_f32, d_x_f32, d_out_f32, n_i64, d_x_i64, d_out_i64_as_f32),
      !d_mul || !d_div ? "null scalar table pointer" : nullptr,
      bad_tables(n_f32, d_x_f32, n_i64, d_x_i64),
      !aligned(d_mul, 4) || !aligned(d_div, 4) ? "scalar tables must be 4-byte aligned" : nullptr,
      bad_outputs(n_f32, d_out_f32, n_i64, d_out_i64_as_f32),
      too_many_coords(n_f32, n_i64),
  });
  if (why) return fail(PLATO_AGG_EINVAL, why);
  if (n_f32)
    hipLaunchKernelGGL((scaled_sum_kernel<false>), dim3(uint32_t((n_f32 + 255) / 256)), dim3(256), 0, stream, d_x_f32,
                       K, d_mul, d_div, post, d_out_f32, uint64_t(n_f32));
  if (n_i64)
    hipLaunchKernelGGL((scaled_sum_kernel<true>), dim3(uint32_t((n_i64 + 255) / 256)), dim3(256), 0, stream, d_x_i64,
                       K, d_mul, d_div, post, d_out_i64_as_f32, uint64_t(n_i64));
  if (n_f32 || n_i64) {
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(PLATO_AGG_EHIP, std::string("scaled_sum: ") + hipGetErrorString(err));
  }
  return plato_agg_internal::clear_error();
}

}  // extern "C"
