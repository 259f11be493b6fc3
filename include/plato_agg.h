/*
 * plato_agg.h — C ABI of the MI355X (gfx950) FedAvg aggregation engine.
 *
 * This is the drop-in boundary for Plato's server-side aggregation hot path.
 * Every entry point takes plain device pointers, element counts and a HIP
 * stream; nothing here allocates device memory, keeps a pointer after it
 * returns, or synchronises the stream (so the calls can be captured in a
 * hipGraph).  Host code (plato_amd/, ctypes) owns all buffers.
 *
 * Arithmetic contract (bit-exact with the reference CPU path):
 *   for every element e, clients i = 0..K-1 in the order of `d_x`:
 *     d   = x_i[e] - b[e]                  (fp32, RNE)       algorithms/fedavg.py:23
 *     t   = d * w_i                        (fp32, RNE)       servers/fedavg.py:154
 *     t   = t * s_i      (only if d_s)     (fp32, RNE)       pisces_server.py:94
 *     acc = acc + t                        (fp32, RNE, acc starts at +0)
 *   new[e] = b[e] + acc                    (fp32, RNE)       algorithms/fedavg.py:35
 * No FMA contraction, no reordering of the K-sum.  int64 entries (BatchNorm
 * num_batches_tracked) follow torch's promotion: d = x - b exactly in int64,
 * converted to fp32 (RNE) before the multiply, new = fp32(b) + acc as fp32;
 * load_state_dict's fp32 -> int64 truncation is plato_agg_cast_f32_i64.
 *
 * Errors: every call returns 0 on success or a negative PLATO_AGG_E* code;
 * plato_agg_last_error() gives a thread-local message for the last failure.
 * (The reference raises Python exceptions; plato_amd/_lib.py maps a non-zero
 * return to RuntimeError/ValueError.)
 *
 * Reference interfaces replaced (TL-System/plato @ 2025-10-03):
 *   plato_agg_fedavg_weights   <- Server._process_reports' deltas -> aggregate
 *                                 -> update chain, i.e. what an
 *                                 `aggregate_weights` hook must return
 *                                 (plato/servers/fedavg.py:171-196,
 *                                  plato/algorithms/fedavg.py:13-37)
 *   plato_agg_fedavg_deltas    <- Server.aggregate_deltas
 *                                 (plato/servers/fedavg.py:137-159)
 *   plato_agg_compute_deltas   <- Algorithm.compute_weight_deltas
 *                                 (plato/algorithms/fedavg.py:13-27)
 *   plato_agg_update_weights   <- Algorithm.update_weights
 *                                 (plato/algorithms/fedavg.py:29-37)
 *   plato_agg_cast_f32_i64     <- Algorithm.load_weights' load_state_dict
 *                                 fp32 -> int64 copy (plato/algorithms/fedavg.py:46-48)
 *   plato_agg_fedavg_weights_bf16 <- the model_dequantize inbound processor
 *                                 (plato/processors/model_dequantize.py:15-18)
 *                                 followed by the same chain, on bf16 payloads
 *   plato_agg_mix_weights      <- FedAsync Algorithm.aggregate_weights
 *                                 (examples/async/fedasync/fedasync_algorithm.py:9-20)
 *   plato_agg_client_dots      <- the model-wide reductions of Port's
 *                                 cosine_similarity (examples/async/port/
 *                                 port_server.py:24-52, F.cosine_similarity over
 *                                 the flattened models)
 *   plato_agg_entry_stats      <- the per-tensor reductions of the norm- and
 *                                 angle-based variants: FedAtt's per-layer
 *                                 torch.linalg.norm (examples/server_aggregation/
 *                                 fedatt/fedatt_algorithm.py:34-39), FedAdp's
 *                                 np.inner / np.linalg.norm of flattened deltas
 *                                 (examples/server_aggregation/fedadp/
 *                                 fedadp_server.py:95-99), Polaris' per-client
 *                                 conv-layer squared deltas (examples/
 *                                 client_selection/polaris/polaris_server.py:76-89)
 *   plato_agg_fedavg_qsgd      <- the model_dequantize_qsgd inbound processor
 *                                 (plato/processors/model_dequantize_qsgd.py:34-60)
 *                                 followed by the FedAvg chain, on QSGD payloads
 *   plato_agg_fedavg_entrywise <- weighted sums whose weight depends on the
 *                                 tensor as well as the client: FedAtt's
 *                                 attentive aggregation (fedatt_algorithm.py:44-69)
 *                                 and FedAdp's global-gradient pass
 *                                 (fedadp_server.py:43-50)
 *   plato_agg_robust_columns   <- the detector example's coordinate-wise median
 *                                 (examples/detector/aggregations.py:55-73) and
 *                                 the mean of the values nearest it that ends its
 *                                 Trimmed-mean and Bulyan (:125-132, :238-243)
 *   plato_agg_pairwise_sqdist, <- the detector example's Multi-Krum: the distance
 *   plato_agg_mean_rows           loop of every selection step and the mean of the
 *                                 selected models (aggregations.py:176-230); the
 *                                 distances serve Bulyan's selection too (:86-123)
 *   plato_agg_trust_stats,     <- the detector example's Fl-trust: the torch.dot /
 *   plato_agg_scaled_sum          torch.norm loop over the clients (aggregations.py:
 *                                 413-423, :432-433) and the scaled candidates and
 *                                 their torch.sum (:428-441); torch.mean (:408) is
 *                                 plato_agg_mean_rows
 *   plato_agg_detect_means,    <- the detector example's FLDetector defence
 *   plato_agg_rows_dots,          (examples/detector/detectors.py:67-106, 310-418):
 *   plato_agg_lbfgs_predict,      the means and record rows of a round, the Gram
 *   plato_agg_delta_sqdist        matrices of lbfgs(), its prediction and the
 *                                 clients' distances to it
 */
#ifndef PLATO_AGG_H
#define PLATO_AGG_H

#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PLATO_AGG_ABI_VERSION 5

#define PLATO_AGG_OK 0
#define PLATO_AGG_EINVAL (-1)   /* bad argument (null, misaligned, K <= 0) */
#define PLATO_AGG_EHIP (-2)     /* HIP runtime error (launch / copy)      */
#define PLATO_AGG_ERCCL (-3)    /* RCCL unavailable or a collective failed */

/* ABI version of the loaded library (== PLATO_AGG_ABI_VERSION). */
int plato_agg_abi_version(void);

/* Thread-local description of the last failure on this thread ("" if none). */
const char* plato_agg_last_error(void);

/*
 * Fused FedAvg over K client weight arenas (a3 -> a4 -> a6 in one pass).
 *   d_x_f32  device array of K pointers, each to n_f32 fp32 client weights
 *            (16-byte aligned); summation order = array order.
 *   d_x_i64  device array of K pointers to n_i64 int64 client entries, or
 *            NULL when n_i64 == 0.
 *   d_w      device array of K fp32 weights (fp32(n_i / N) for FedAvg).
 *   d_s      device array of K fp32 second scalars, or NULL.
 *   d_base_* the global model (baseline) entries.
 *   d_out_f32   n_f32 fp32 new weights (may alias d_base_f32).
 *   d_out_i64f  n_i64 fp32 new values of the int64 entries (the reference's
 *               update_weights yields fp32 for them; cast with
 *               plato_agg_cast_f32_i64 to get what load_state_dict stores).
 */
int plato_agg_fedavg_weights(const float* const* d_x_f32,
                             const int64_t* const* d_x_i64,
                             const float* d_w, const float* d_s, int K,
                             const float* d_base_f32, const int64_t* d_base_i64,
                             float* d_out_f32, float* d_out_i64f,
                             size_t n_f32, size_t n_i64, hipStream_t stream);

/*
 * Weighted sum of K client delta arenas (Server.aggregate_deltas):
 *   avg[e] = sum_i fp32(d_i[e]) * w_i  (sequential, fp32), avg is fp32 for
 * every entry, including the int64 ones (trainers/basic.py:59-63).
 */
int plato_agg_fedavg_deltas(const float* const* d_d_f32,
                            const int64_t* const* d_d_i64,
                            const float* d_w, const float* d_s, int K,
                            float* d_avg_f32, float* d_avg_i64f,
                            size_t n_f32, size_t n_i64, hipStream_t stream);

/*
 * Fused FedAvg over K bf16-quantized client payloads (Plato's model_quantize
 * codec: every entry .to(bfloat16), plato/processors/model_quantize.py:15),
 * equal to dequantizing them on the server (model_dequantize.py:15-18,
 * .to(float32), exact) and running plato_agg_fedavg_weights: the payload
 * stays bf16 through PCIe and HBM and is widened in registers.  The int64
 * entries' payload values are bf16 as well; as in the reference, they are
 * subtracted from the int64 baseline in fp32: d = fp32(x) - fp32(b).
 *   d_x_bf16      K pointers to n_f32 bf16 values (16-byte aligned)
 *   d_x_i64_bf16  K pointers to n_i64 bf16 values (or NULL if n_i64 == 0)
 * Other arguments as plato_agg_fedavg_weights.
 */
int plato_agg_fedavg_weights_bf16(const uint16_t* const* d_x_bf16,
                                  const uint16_t* const* d_x_i64_bf16,
                                  const float* d_w, const float* d_s, int K,
                                  const float* d_base_f32, const int64_t* d_base_i64,
                                  float* d_out_f32, float* d_out_i64f,
                                  size_t n_f32, size_t n_i64, hipStream_t stream);

/* One client's deltas: out = x - base (fp32), and exact int64 x - base. */
int plato_agg_compute_deltas(const float* d_x_f32, const int64_t* d_x_i64,
                             const float* d_base_f32, const int64_t* d_base_i64,
                             float* d_out_f32, int64_t* d_out_i64,
                             size_t n_f32, size_t n_i64, hipStream_t stream);

/* update_weights: out = base + avg (fp32; int64 base converted to fp32). */
int plato_agg_update_weights(const float* d_base_f32, const int64_t* d_base_i64,
                             const float* d_avg_f32, const float* d_avg_i64f,
                             float* d_out_f32, float* d_out_i64f,
                             size_t n_f32, size_t n_i64, hipStream_t stream);

/*
 * load_state_dict's fp32 -> int64 copy: truncation toward zero; NaN and
 * values outside [-2^63, 2^63) give INT64_MIN (the x86-64 conversion result
 * the reference CPU path produces).
 */
int plato_agg_cast_f32_i64(const float* d_src, int64_t* d_dst, size_t n,
                           hipStream_t stream);

/*
 * FedAsync mixing: out = fp32(b * fp32(1 - m)) + fp32(x * fp32(m)), computed
 * as the reference does with two fp32 scalars one_minus_m and m.
 */
int plato_agg_mix_weights(const float* d_x_f32, const int64_t* d_x_i64,
                          const float* d_base_f32, const int64_t* d_base_i64,
                          float one_minus_m, float m,
                          float* d_out_f32, float* d_out_i64f,
                          size_t n_f32, size_t n_i64, hipStream_t stream);

/*
 * Per-client model-wide reductions (Port cosine similarity, norms) over the
 * whole arena, int64 entries included as torch.cat promotes them (fp32):
 *   d_i = x_i - base (fp32, as compute_weight_deltas; int64: fp32(x - b)),
 *         or x_i if d_base is NULL
 *   d_out[i]     = sum_e d_i[e] * v[e]         (0 <= i < K)
 *   d_out[K + i] = sum_e d_i[e]^2
 *   d_out[2K]    = sum_e v[e]^2                (v's int64 entries as fp32)
 * accumulated in fp64 in a fixed order (bitwise reproducible run to run; it
 * matches torch's fp32 CPU reductions within tolerance, not bit for bit).
 * d_workspace must hold plato_agg_client_dots_workspace(K, n_f32) bytes.
 */
size_t plato_agg_client_dots_workspace(int K, size_t n_f32);
int plato_agg_client_dots(const float* const* d_x, const int64_t* const* d_x_i64, int K,
                          const float* d_base, const int64_t* d_base_i64,
                          const float* d_v, const int64_t* d_v_i64,
                          size_t n_f32, size_t n_i64, double* d_workspace,
                          double* d_out, hipStream_t stream);

/*
 * Per-entry work: a state_dict entry ("tensor") is a contiguous element range
 * of the fp32 or the int64 arena.  Kernels that need the entry of an element
 * read a chunk table: each chunk is a piece of ONE entry, [begin, end) in
 * elements of its region, numbered with the entry's index `entry` in the
 * layout (0 <= entry < n_entries, across both regions).  Chunks of the same
 * entry are contiguous and the tables are sorted by entry (host-built once
 * per layout: plato_amd/arena.py ArenaLayout.chunk_tables).  Chunk length
 * sets the work per workgroup; any length is correct.
 */
typedef struct plato_agg_chunk {
  uint32_t entry;
  uint32_t begin;
  uint32_t end;
  uint32_t reserved;
} plato_agg_chunk;

/*
 * Per (client, entry) reductions, accumulated in fp64 in a fixed order:
 *   d_i = x_i - base (fp32; int64 entries: fp32(int64 x - b)), or x_i if d_base is NULL
 *   d_out[i * E + e]           = sum_{elements of e} d_i * v     (0 <= i < K; 0 if d_v is NULL)
 *   d_out[(K + i) * E + e]     = sum d_i^2
 *   d_out[2K * E + e]          = sum v^2                         (0 if d_v is NULL)
 * v is an fp32 arena (its int64 entries given as fp32 in d_v_i64f).
 * d_workspace must hold plato_agg_entry_stats_workspace(K, n_chunks_f32 + n_chunks_i64) bytes.
 */
size_t plato_agg_entry_stats_workspace(int K, uint32_t n_chunks);
int plato_agg_entry_stats(const float* const* d_x_f32, const int64_t* const* d_x_i64, int K,
                          const float* d_base_f32, const int64_t* d_base_i64,
                          const float* d_v_f32, const float* d_v_i64f,
                          const plato_agg_chunk* d_chunks_f32, uint32_t n_chunks_f32,
                          const plato_agg_chunk* d_chunks_i64, uint32_t n_chunks_i64,
                          int n_entries, size_t n_f32, size_t n_i64,
                          double* d_workspace, double* d_out, hipStream_t stream);

/*
 * Weighted sum with a weight per (entry, client), bit-exact with torch's fp32
 * CPU ops:
 *   d_i = x_i - b (as above), or x_i if d_base is NULL
 *   acc = +0; for i in order: acc = acc + fp32(d_i * W[e * K + i])
 *   u   = fp32(acc * scale); if d_noise: u = fp32(u + fp32(noise * noise_scale))
 *   out = (flags & PLATO_AGG_ADD_BASE) ? fp32(b + u) : u      (int64 b: fp32(b) + u)
 * FedAtt: W = -softmax(norms), scale = -epsilon, noise = torch.randn draws,
 * noise_scale = magnitude, ADD_BASE (update_weights).  d_base is required
 * with ADD_BASE.  Alignment: base/out/noise fp32 arrays 16-byte aligned.
 */
#define PLATO_AGG_ADD_BASE 1
int plato_agg_fedavg_entrywise(const float* const* d_x_f32, const int64_t* const* d_x_i64, int K,
                               const float* d_w, int n_entries,
                               const plato_agg_chunk* d_chunks_f32, uint32_t n_chunks_f32,
                               const plato_agg_chunk* d_chunks_i64, uint32_t n_chunks_i64,
                               const float* d_base_f32, const int64_t* d_base_i64,
                               const float* d_noise_f32, const float* d_noise_i64f,
                               float scale, float noise_scale, int flags,
                               float* d_out_f32, float* d_out_i64f,
                               size_t n_f32, size_t n_i64, hipStream_t stream);

/*
 * torch.linalg.norm of every (client, entry) delta, in x86-64 PyTorch's CPU
 * order (ATen's vectorised 2-norm: 8 fp32 lanes of fma(v, v, acc) over the
 * first n - n%8 elements, lanes added in order, tail fma'd, fp32 sqrt), so
 * the fp32 result equals the reference's bit for bit:
 *   d_out[i * n_entries + entry] = norm(d_i restricted to entry)
 * A one-element entry (any shape with numel == 1, () included) gives |d|, as
 * torch does: no square is formed, so |d| below 1.1e-19 or above 1.8e19 comes
 * back as it is where sqrt(d * d) would give 0, a rounded value or inf.  From
 * two elements on NaN, +-inf, subnormal squares and sums that overflow follow
 * the chain's IEEE arithmetic (pinned at such values against torch through
 * oracle/reductions.c: tests/test_reductions.py, tests/test_special_values_gpu.py).
 * d_entries_* hold ONE piece per entry (ArenaLayout.chunk_tables(2**32)), in
 * any order: the table order is the dispatch order, and since each norm is one
 * serial chain, passing the longest entries first shortens the launch (the
 * engine does, FedAvgEngine._norm_tables).
 * FedAtt: examples/server_aggregation/fedatt/fedatt_algorithm.py:34-39.
 */
int plato_agg_entry_norms_f32(const float* const* d_x_f32, const int64_t* const* d_x_i64, int K,
                              const float* d_base_f32, const int64_t* d_base_i64,
                              const plato_agg_chunk* d_entries_f32, uint32_t n_entries_f32,
                              const plato_agg_chunk* d_entries_i64, uint32_t n_entries_i64,
                              int n_entries, size_t n_f32, size_t n_i64, float* d_out,
                              hipStream_t stream);

/*
 * FedAvg over QSGD-coded payloads (one byte per element: bit 7 sign, bits
 * 0-6 |zeta|; one max_v per (entry, client)), decoded exactly as
 * model_dequantize_qsgd.py:51-58 does before the FedAvg chain:
 *   x   = fp32(fp32(fp32(zeta) * max_v[entry * K + i]) / divisor)   (divisor = level - 1)
 *   d   = x - b   (int64 entries: x - fp32(b)),  t = fp32(d * w_i) [* s_i],  acc += t
 *   out = fp32(b + acc)     (int64 entries: fp32(b) + acc)
 * d_codes_* are K device pointers to byte arenas laid out like the fp32 /
 * int64 regions (element e <-> byte e), 16-byte aligned.  Chunk tables as
 * for plato_agg_fedavg_entrywise (pieces of <= 4096 elements run one pass).
 */
int plato_agg_fedavg_qsgd(const uint8_t* const* d_codes_f32, const uint8_t* const* d_codes_i64, int K,
                          const float* d_max_v, int n_entries, float divisor,
                          const float* d_w, const float* d_s,
                          const plato_agg_chunk* d_chunks_f32, uint32_t n_chunks_f32,
                          const plato_agg_chunk* d_chunks_i64, uint32_t n_chunks_i64,
                          const float* d_base_f32, const int64_t* d_base_i64,
                          float* d_out_f32, float* d_out_i64f, size_t n_f32, size_t n_i64,
                          hipStream_t stream);

/*
 * Deterministic synthetic payloads for tests and benchmarks (a counter-based
 * generator restated bit for bit by oracle/synth.py):
 *   h = splitmix64(splitmix64(seed ^ (stream * 0xD1B54A32D192ED03)) + e)
 *   r = (int32)(h >> 40) - 2^23
 *   out[e] = (d_add ? d_add[e] : +0) + (float)r * 2^scale_log2   (fp32 add)
 */
int plato_agg_fill_synth_f32(float* d_out, const float* d_add, size_t n,
                             uint64_t seed, uint64_t stream_id, int scale_log2,
                             hipStream_t stream);

/*   out[e] = (d_add ? d_add[e] : 0) + (int64)(h % modulus)   (modulus >= 1) */
int plato_agg_fill_synth_i64(int64_t* d_out, const int64_t* d_add, size_t n,
                             uint64_t seed, uint64_t stream_id, uint64_t modulus,
                             hipStream_t stream);

/*
 * The same streams from element ``first`` on: out[e] is element first + e of
 * the stream (h = splitmix64(key + first + e)) and d_add[e] its addend.  A
 * rank of the bucket-sharded bench fills its pieces as slices of the one
 * global model and client set this way (bench.py, N > 1).
 */
int plato_agg_fill_synth_f32_at(float* d_out, const float* d_add, size_t n,
                                uint64_t seed, uint64_t stream_id, uint64_t first,
                                int scale_log2, hipStream_t stream);
int plato_agg_fill_synth_i64_at(int64_t* d_out, const int64_t* d_add, size_t n,
                                uint64_t seed, uint64_t stream_id, uint64_t first,
                                uint64_t modulus, hipStream_t stream);

/*
 * FedAvg with float64 weights on the fp32 entries (ABI 2): for every fp32
 * element, clients in order,
 *   d = x_i - b (fp32; d = x_i when d_base_* are NULL: deltas mode)
 *   acc = fp32( double(acc) + double(d) * d_w64[i] )      (one double rounding
 *         for the product, one for the sum, then the cast: torch's in-place add
 *         of a float64 tensor into an fp32 one)
 *   new = fp32(b + acc)            (deltas mode: acc)
 * and for the int64 entries the fp32 chain with d_w_i64[i] (fp32):
 *   acc = acc + fp32(fp32(x_i - b) * w_i64),  new = fp32(b) + acc.
 * Replaces the RL server's smart weighting (plato/utils/reinforcement_learning/
 * rl_server.py:66-71: `delta * smart_weighting[i]` with a float64 [K, 1]
 * action for the fp32 entries, `delta * smart_weighting[i][0]` for the int64
 * ones).  Arena < 4 GiB per call.
 */
int plato_agg_fedavg_w64(const float* const* d_x_f32, const int64_t* const* d_x_i64, const double* d_w64,
                         const float* d_w_i64, int K, const float* d_base_f32, const int64_t* d_base_i64,
                         float* d_out_f32, float* d_out_i64f, size_t n_f32, size_t n_i64, hipStream_t stream);

/*
 * float64 weighted sum of K float64 vectors (16-byte aligned):
 *   out[e] = (((0 + x_0[e]*w_0) + x_1[e]*w_1) + ...)   float64, separately rounded.
 * The plaintext half of HE hybrid FedAvg (plato/servers/fedavg_he.py:88-98):
 * the unencrypted weights are float64 numpy vectors (homo_enc.py:50-63), so
 * `unencrypted_avg_update += unenc_w * (n_i / N)` runs in numpy float64 and
 * turns the fp32 zeros into a float64 accumulator.
 */
int plato_agg_weighted_sum_f64(const double* const* d_x, const double* d_w, int K, double* d_out, size_t n,
                               hipStream_t stream);

/*
 * Flattened-model reductions of the variant servers, in the reference's own
 * float32 order (bit-exact; CPU restatements in oracle/reductions.c).
 *
 * plato_agg_flatten writes K flat fp32 vectors: position p of vector k lies in
 * segment s (the last with flat_offset <= p), element e = src_offset +
 * (p - flat_offset) of its region, and is
 *   PLATO_AGG_FLAT_DELTA      fp32: x_k[e] - b[e];   int64: fp32(x_k[e] - b[e])
 *   PLATO_AGG_FLAT_CAST_DIFF  fp32: x_k[e] - b[e];   int64: fp32(x_k[e]) - fp32(b[e])
 *   PLATO_AGG_FLAT_RAW        fp32: x_k[e];          int64 region given as fp32 values
 * and, with PLATO_AGG_SEG_NEG_DIV, (-v) / lr instead (int64 deltas: the int64
 * negation, then the cast and the division).  Port concatenates the entries in
 * state_dict order (examples/async/port/port_server.py:36-48, CAST_DIFF for
 * current - previous, DELTA for the update); FedAdp sorts them by name.lower()
 * and divides all but the first by -lr (examples/server_aggregation/fedadp/
 * fedadp_server.py:122-133, RAW for the global gradient, DELTA for a client).
 * d_src_*: K device pointers; d_out: K device pointers to n_flat floats.
 * Delta arenas: in PLATO_AGG_FLAT_DELTA, d_base_f32 = d_base_i64 = NULL means the
 * sources already hold x - b (fp32 differences, int64 wrapping differences:
 * compute_weight_deltas, plato/algorithms/fedavg.py:13-27, formed when each payload
 * was staged); the values are the same (x - (+0) for fp32, x - 0 for int64), and the
 * kernel reads no baseline.  One of the two NULL, or a NULL baseline in
 * PLATO_AGG_FLAT_CAST_DIFF, is PLATO_AGG_EINVAL.
 */
typedef struct plato_agg_segment {
  uint64_t flat_offset;
  uint64_t src_offset;
  uint64_t numel;
  uint32_t region;  /* 0: fp32 region, 1: int64 region */
  uint32_t flags;   /* PLATO_AGG_SEG_NEG_DIV */
} plato_agg_segment;
#define PLATO_AGG_FLAT_DELTA 0
#define PLATO_AGG_FLAT_CAST_DIFF 1
#define PLATO_AGG_FLAT_RAW 2
#define PLATO_AGG_SEG_NEG_DIV 1u
int plato_agg_flatten(int mode, const void* const* d_src_f32, const void* const* d_src_i64, int K,
                      const float* d_base_f32, const int64_t* d_base_i64, const plato_agg_segment* d_segs,
                      uint32_t n_segs, size_t n_flat, float lr, float* const* d_out, hipStream_t stream);

/*
 * numpy's float32 np.inner(x_j, y_j) (and y_j . y_j if d_out_yy) for n_pairs
 * pairs of flat vectors, in the order of numpy's bundled OpenBLAS 0.3.29
 * sdot_k_SKYLAKEX (the x86-64 AVX-512 kernel; cblas_sdot calls it unthreaded):
 * FedAdp's inner products and norms (fedadp_server.py:95-99; np.linalg.norm
 * is sqrt of the float32 self dot).  Vectors 16-byte aligned.
 * n == 1: the kernels return +0 + x[0] * y[0], numpy the bare product, so a
 * product of -0 comes back as +0 here and as -0 there (equal by value; the
 * only departure, and only in the sign of zero).  FedAdp, the one consumer,
 * takes arccos(clip(inner / norms)), which gives the same bits for both zeros.
 * The same holds for plato_agg_sdot_shared and plato_agg_fedadp_dots.
 */
int plato_agg_sdot_pairs(const float* const* d_x, const float* const* d_y, int n_pairs, size_t n,
                         float* d_out_xy, float* d_out_yy, hipStream_t stream);

/*
 * The same sdot_k_SKYLAKEX results (bitwise equal to plato_agg_sdot_pairs) for
 * pairs that share x: FedAdp's np.inner(g, loc_k) and loc_k . loc_k for every
 * client (fedadp_server.py:91-99); with with_xx = 1 also g . g, written to
 * d_out_xy[n_pairs] and d_out_yy[n_pairs].  The 64 chains are split over
 * workgroups and each workgroup reads x once for its pairs; d_workspace holds
 * plato_agg_sdot_shared_workspace(n_pairs, with_xx) bytes of chain partials.
 * x 16-byte aligned; y rows any float alignment.
 */
size_t plato_agg_sdot_shared_workspace(int n_pairs, int with_xx);
int plato_agg_sdot_shared(const float* d_x, const float* const* d_y, int n_pairs, size_t n, int with_xx,
                          float* d_workspace, float* d_out_xy, float* d_out_yy, hipStream_t stream);

/*
 * FedAdp's dots straight from the staged arenas, bit-equal to plato_agg_flatten
 * (PLATO_AGG_FLAT_DELTA with the segment map) followed by plato_agg_sdot_shared,
 * without the flattened copies: process_grad(update) positions are gathered
 * through d_segs (flat order: entries sorted by name.lower(), NEG_DIV on all but
 * the first) from client k's arenas d_src_f32[k] / d_src_i64[k] and the baseline
 * (loc = x - b, or -(x - b) / lr), and d_out_xy[k] = np.inner(x, loc_k),
 * d_out_yy[k] = loc_k . loc_k in numpy's OpenBLAS sdot_k_SKYLAKEX order
 * (examples/server_aggregation/fedadp/fedadp_server.py:91-99, 122-133).  d_x is
 * the flattened global gradient (plato_agg_flatten RAW, 16-byte aligned, at
 * least n_flat rounded up to 64 floats); with_xx = 1 also writes x . x to
 * d_out_xy[n_pairs] and d_out_yy[n_pairs].  Segments: 1 .. 2^22 - 1 (ABI 3: no
 * longer capped at 2048 entries), n_flat < 2^30, n_pairs <= 65535; n_f32 / n_i64 =
 * lengths of the arenas' fp32 (< 2^30) and int64 regions.  d_workspace (256-byte
 * aligned): plato_agg_fedadp_dots_workspace(n_pairs, with_xx, n_i64, n_flat,
 * n_segs) bytes — chain sums, per-group descriptors, the finished values of
 * the groups that cross an entry boundary and the chain-group-major copy of x
 * and the flattened baseline the kernel streams.
 * Delta arenas: d_base_f32 = d_base_i64 = NULL means the client arenas already
 * hold x - b (fp32 differences, int64 wrapping differences: compute_weight_deltas,
 * plato/algorithms/fedavg.py:13-27, formed when each payload was staged); the
 * values and their order are the same, and the kernel streams no baseline.
 */
size_t plato_agg_fedadp_dots_workspace(int n_pairs, int with_xx, size_t n_i64, size_t n_flat, uint32_t n_segs);
int plato_agg_fedadp_dots(const float* d_x, const void* const* d_src_f32, const void* const* d_src_i64, int n_pairs,
                          const float* d_base_f32, const int64_t* d_base_i64, const plato_agg_segment* d_segs,
                          uint32_t n_segs, size_t n_flat, size_t n_f32, size_t n_i64, float lr, int with_xx, void* d_workspace,
                          float* d_out_xy, float* d_out_yy, hipStream_t stream);

/*
 * plato_agg_fedadp_dots with flags (ABI 4).  PLATO_AGG_FEDADP_TABLES_READY: d_workspace
 * already holds the layout-only tables (per-group descriptors, boundary rows and their
 * source positions) of an earlier call with the same d_segs contents, n_segs, n_flat,
 * n_i64, n_pairs and with_xx, completed on or ordered before `stream`; they depend on
 * the segment map only, so a server whose layout is unchanged between rounds builds
 * them once (replaces nothing in the reference: the same dots as plato_agg_fedadp_dots,
 * examples/server_aggregation/fedadp/fedadp_server.py:91-99).  flags = 0 is
 * plato_agg_fedadp_dots.
 */
#define PLATO_AGG_FEDADP_TABLES_READY 1
int plato_agg_fedadp_dots_ex(const float* d_x, const void* const* d_src_f32, const void* const* d_src_i64,
                             int n_pairs, const float* d_base_f32, const int64_t* d_base_i64,
                             const plato_agg_segment* d_segs, uint32_t n_segs, size_t n_flat, size_t n_f32,
                             size_t n_i64, float lr, int with_xx, void* d_workspace, float* d_out_xy, float* d_out_yy,
                             hipStream_t stream, int flags);

/*
 * Port's vector norms gathered from the arenas (replaces the flatten + norm of
 * examples/async/port/port_server.py:38-50: torch.cat in state_dict order, then
 * the norms inside F.cosine_similarity).  Vector v is x_v - b_v flattened by
 * the segment map (state_dict order; int64 entries cast to float32 as
 * torch.cat does: the wrapped int64 difference cast once, or with
 * PLATO_AGG_PORT_CAST_FIRST for vector 0, current - previous, the difference
 * of the two casts); d_out[v] = torch.linalg.vector_norm of it in x86-64
 * ATen's order (8 fma chains over n - n % 8 positions, the lanes added in
 * order, the scalar tail); a vector of one position (n_flat == 1 or
 * d_lengths[v] == 1) gives |d|, as torch does for a one-element tensor (no
 * square, see plato_agg_entry_norms_f32).  d_x_f32 / d_x_i64 / d_b_f32 / d_b_i64: n_vectors
 * device pointers each (arenas of n_f32 fp32 elements / the int64 counters).
 * d_flat_out: null, or n_vectors 16-byte aligned rows of >= n_flat floats that
 * receive the flattened vectors (what plato_agg_torch_cosine_sum then reads).
 * d_lengths: null, or n_vectors lengths <= n_flat, vector v taking only its
 * first d_lengths[v] positions (FedAtt's per-(entry, client) norms,
 * fedatt_algorithm.py:34-39: one fp32 entry of one client per vector, the
 * pointers offset to the entry and one segment covering it).  A null
 * d_b_f32[v] (and d_b_i64[v]) means vector v's arenas already hold the
 * difference (delta arenas): nothing is subtracted, the same values result.
 */
#define PLATO_AGG_PORT_CAST_FIRST 1
int plato_agg_port_norms(const void* const* d_x_f32, const void* const* d_x_i64, const void* const* d_b_f32,
                         const void* const* d_b_i64, int n_vectors, const uint32_t* d_lengths,
                         const plato_agg_segment* d_segs, uint32_t n_segs, size_t n_flat, size_t n_f32, int flags,
                         float* d_out, float* const* d_flat_out, hipStream_t stream);

/*
 * The sum in Port's F.cosine_similarity(a, b_k, dim=0) (port_server.py:50),
 * as x86-64 PyTorch 2.10 forms it on `threads` CPU threads:
 *   q = (a / max(|a|, eps)) * (b_k / max(|b_k|, eps)),  out[k] = sum(q)
 * in TensorIterator's two-pass order (min(threads, ceil(n/32768)) chunks;
 * one pass below 32768 elements or on one thread), each chunk by ATen's
 * cascade sum.  |a|, |b_k|: device floats, e.g. plato_agg_entry_norms_f32 of
 * the flat vectors with no baseline (torch.linalg.vector_norm's order).
 * d_workspace: plato_agg_torch_cosine_workspace(K, threads) bytes.
 */
size_t plato_agg_torch_cosine_workspace(int K, int threads);
int plato_agg_torch_cosine_sum(const float* d_a, const float* const* d_b, int K, size_t n, const float* d_norm_a,
                               const float* d_norm_b, float eps, int threads, void* d_workspace, float* d_out,
                               hipStream_t stream);

/*
 * plato_agg_torch_cosine_sum with a already divided by its clamped norm
 * (F.cosine_similarity's x1 / x1_norm, the same fp32 quotients: one division
 * per element and client instead of two).  plato_agg_scale_by_norm forms it:
 * d_out[i] = d_a[i] / max(*d_norm, eps) (NaN norms stay NaN).
 */
int plato_agg_torch_cosine_sum_scaled(const float* d_a_scaled, const float* const* d_b, int K, size_t n,
                                      const float* d_norm_b, float eps, int threads, void* d_workspace, float* d_out,
                                      hipStream_t stream);
int plato_agg_scale_by_norm(const float* d_a, size_t n, const float* d_norm, float eps, float* d_out,
                            hipStream_t stream);

/*
 * numpy's float32 np.sum(np.square(x_k - b)) of each fp32 piece (one per
 * entry, d_pieces rows (entry, begin, end)): the ufunc reduction's 8192-element
 * inner loops, out += pairwise_sum(chunk) from 0, pairwise_sum as numpy's
 * (8 partial sums up to 128 elements, halved at multiples of 8 above).
 * Polaris' per-layer squared deltas (examples/client_selection/polaris/
 * polaris_server.py:78-81).  d_first_chunk[p] = sum over earlier pieces of
 * ceil(len / 8192); n_chunks the total.  d_out: [K][n_pieces] floats.
 * d_workspace: plato_agg_np_sumsq_workspace(K, n_chunks) bytes (the per-chunk sums).
 */
size_t plato_agg_np_sumsq_workspace(int K, uint32_t n_chunks);
int plato_agg_np_sumsq(const float* const* d_x, int K, const float* d_base, const plato_agg_chunk* d_pieces,
                       const uint32_t* d_first_chunk, uint32_t n_pieces, uint32_t n_chunks, void* d_workspace,
                       float* d_out, hipStream_t stream);

/*
 * Coded client payloads (or the baseline) as fp32 rows of the "promoted"
 * layout, for the variant servers' per-entry reductions: what the reference's
 * inbound dequantizers hand the server (plato/processors/model_dequantize.py:
 * 15-18, model_dequantize_qsgd.py:34-60), every entry float32 — the int64
 * counters included, so a counter's delta is float32(x) - float32(b).
 *   PLATO_AGG_DECODE_NATIVE  fp32 copied, int64 cast to fp32 (RNE)
 *   PLATO_AGG_DECODE_BF16    bf16 widened (exact), both regions
 *   PLATO_AGG_DECODE_QSGD    fp32(fp32(fp32(zeta) * max_v[entry][k]) / divisor)
 * Element e of the fp32 region lands at d_dst[k][e], element e of the int64
 * region at d_dst[k][i64_dst_offset + e]; pieces from d_chunks_* (entry, begin,
 * end); d_max_v: [n_entries][K] (QSGD only).
 */
#define PLATO_AGG_DECODE_NATIVE 0
#define PLATO_AGG_DECODE_BF16 1
#define PLATO_AGG_DECODE_QSGD 2
int plato_agg_decode_rows(int codec, const void* const* d_src_f32, const void* const* d_src_i64, int K,
                          const float* d_max_v, float divisor, const plato_agg_chunk* d_chunks_f32,
                          uint32_t n_chunks_f32, const plato_agg_chunk* d_chunks_i64, uint32_t n_chunks_i64,
                          size_t i64_dst_offset, float* const* d_dst, hipStream_t stream);

/*
 * Coordinate-wise robust aggregation over K client arenas: the order statistics
 * of the reference's Byzantine-robust aggregators (examples/detector/
 * aggregations.py, reached through detector_server.Server.aggregate_weights and
 * server.secure_aggregation_type), which are not weighted sums.
 *   PLATO_AGG_ROBUST_MEDIAN   aggregations.median: torch.median(X, dim=0)[0] of
 *                             the flattened [K, d] matrix.
 * Per coordinate j the column is c_k = x_k[j]; for the int64 region it is
 * (float)x_k[j], round to nearest even (flatten_weights' torch.cat promotes the
 * counters to fp32), and the result is fp32 there too.
 *   median: NaN if any c_k is NaN, else the element at index (K-1)/2 of the
 *   ascending order (torch's lower median).  +-inf and subnormals are ordinary
 *   values (no flush to zero).  -0 and +0 compare equal in the reference, where
 *   the one returned is an implementation accident; here the order is total,
 *   -0 < +0 (the one documented divergence).  A selection: no rounding.
 *   PLATO_AGG_ROBUST_NEAREST_MEAN   the last step of aggregations.trimmed_mean and
 *                             aggregations.bulyan: the mean of the b = K - 2*trim
 *                             values of the column nearest its lower median,
 *                               med = torch.median(X, dim=0)[0]
 *                               idx = torch.argsort(torch.abs(X - med), dim=0)
 *                               torch.mean(X[idx, arange(d)][:b], dim=0)
 *   nearest mean: NaN (0x7fc00000) if any c_k is NaN.  Else med is the median
 *   above and d_k = |c_k - med|: one separately rounded fp32 subtraction with the
 *   sign bit cleared; a NaN distance (inf - inf) becomes 0x7fc00000.  The unsigned
 *   bit pattern of d_k is its key: 0 < ... < +inf < NaN, both zeros are key 0.
 *   T is the key of rank b-1, ascending.  Every row with key < T is kept, and the
 *   rows with key == T in table order until b rows are kept ("lowest table
 *   position"; the reference's argsort is not stable, so which of two equally
 *   distant values it keeps is an accident: a documented divergence).  acc = +0;
 *   for the kept rows in table order acc = acc + c_k, each add rounded in fp32;
 *   the result is acc / (float)b by IEEE division.  Only the set of kept values
 *   enters, not their order by distance: torch.mean's blocked sum differs from
 *   this sequential one by rounding only.  With trim == 0 the result is bit for
 *   bit that of plato_agg_mean_rows on the same table.
 *   d_x_f32  device array of K pointers, each to n_f32 fp32 values
 *   d_x_i64  device array of K pointers to n_i64 int64 values, or NULL when
 *            n_i64 == 0
 *   trim     0 <= 2*trim < K in both modes; the median ignores it otherwise
 *   d_out_f32 (16-byte aligned), d_out_i64_as_f32: the results
 * 1 <= K <= PLATO_AGG_ROBUST_MAX_K.  Any other mode is PLATO_AGG_EINVAL.
 */
#define PLATO_AGG_ROBUST_MEDIAN 0
#define PLATO_AGG_ROBUST_NEAREST_MEAN 1
#define PLATO_AGG_ROBUST_MAX_K 256
int plato_agg_robust_columns(int mode, const float* const* d_x_f32, const int64_t* const* d_x_i64, int K,
                             int trim, float* d_out_f32, float* d_out_i64_as_f32, size_t n_f32, size_t n_i64,
                             hipStream_t stream);

/*
 * Multi-Krum (examples/detector/aggregations.py:176-230, "Multi-krum" of
 * server.secure_aggregation_type): the K x K squared L2 distances over the whole
 * flattened model, a selection on the host (plato_amd/krum.py), and the mean of
 * the selected rows.  "Bulyan" (aggregations.py:76-144) is the same distances,
 * its own selection on the host (plato_amd/krum.py: bulyan_select) and
 * plato_agg_robust_columns(PLATO_AGG_ROBUST_NEAREST_MEAN) over the selected rows.
 * "Krum" is not provided.
 *
 * plato_agg_pairwise_sqdist  <- the distance loop of every selection step
 *                               (aggregations.py:185-192):
 *                                 torch.norm((remaining - weight), dim=1) ** 2
 *                               for every remaining weight, once for all K rows.
 *   d_out[i*K + j] = sum over e of fp32(c_i[e] - c_j[e])^2, over both regions, with
 *   c_k[e] = x_k[e] in the fp32 region and (float)x_k[e] (round to nearest even)
 *   in the int64 region, as flatten_weights' torch.cat promotes the counters.
 *   Each difference is one separately rounded fp32 subtraction (the reference's
 *   `remaining - weight`); never the Gram form |a|^2 + |b|^2 - 2ab, which cancels
 *   what the selection needs when clients are a common model plus small noise.
 *   The squares are accumulated per lane by __fmaf_rn chains of at most
 *   PLATO_AGG_PAIRDIST_CHAIN terms; chain results are added in float64, in a fixed
 *   order: across the lanes of a wave, over the chains of a workgroup's
 *   coordinate chunk, then over the chunks (through d_workspace, by a final
 *   kernel).  No atomics.  |d_out - exact sum of the fp32 differences' squares|
 *   <= ((PLATO_AGG_PAIRDIST_CHAIN + 1) * 2^-24 + D * 2^-53) * d_out, D = n_f32 + n_i64
 *   (the reference's own fp32 sum is within D * 2^-24).
 *   Properties: (a) bitwise repeatable from run to run; (b) d_out[i][j] depends
 *   only on rows i and j and on (n_f32, n_i64), not on K, on where the pair falls
 *   in the tiling or on the order of the pointer table: a permuted table gives
 *   the bitwise permuted matrix, and d_out[i][j] == d_out[j][i] bitwise; (c) the
 *   diagonal is exactly +0, whatever row i holds; (d) off the diagonal NaN and
 *   +-inf propagate by IEEE rules (inf - inf = NaN).
 *   d_x_f32, d_x_i64   device arrays of K row pointers (d_x_i64 NULL when n_i64 == 0)
 *   d_workspace        plato_agg_pairwise_sqdist_workspace(K, n_f32, n_i64) bytes
 *                      (0: bad arguments), 256-byte aligned
 *   d_out              K * K doubles, row-major, 16-byte aligned
 *   1 <= K <= PLATO_AGG_ROBUST_MAX_K; fewer than 2^38 coordinates per region.
 *
 * plato_agg_mean_rows  <- torch.mean(candidates, dim=0) (aggregations.py:218)
 *   for every coordinate e: acc = +0; for r = 0..m-1 in table order:
 *   acc = acc + c_r[e] (fp32, separately rounded); out[e] = acc / (float)m (IEEE
 *   division).  fp32 results for both regions.  1 <= m <= 256.
 *
 * Two documented divergences from the reference, both by rounding or by an
 * accident of the reference only:
 *   - the mean is the sequential row sum over m; torch.mean on the CPU is
 *     torch.sum(X, dim=0) / fp32(m) with ATen's blocked row order, which equals
 *     the sequential sum only for small m.  Both are within the any-order
 *     summation bound 2(m-1) * 2^-24 * sum|x| / m of each other.
 *   - the selection breaks score ties towards the lowest client index (the
 *     reference's torch.argsort is not stable).
 */
#define PLATO_AGG_PAIRDIST_CHAIN 128
size_t plato_agg_pairwise_sqdist_workspace(int K, size_t n_f32, size_t n_i64);
int plato_agg_pairwise_sqdist(const float* const* d_x_f32, const int64_t* const* d_x_i64, int K,
                              size_t n_f32, size_t n_i64, void* d_workspace,
                              double* d_out /* K*K, row-major */, hipStream_t stream);
int plato_agg_mean_rows(const float* const* d_x_f32, const int64_t* const* d_x_i64, int m,
                        float* d_out_f32, float* d_out_i64_as_f32,
                        size_t n_f32, size_t n_i64, hipStream_t stream);

/*
 * Fl-trust (examples/detector/aggregations.py:403-453, "Fl-trust" of
 * server.secure_aggregation_type): the cosine of every client with the mean model,
 * clipped at 0 and normalised, weighs the clients, each rescaled to the mean's
 * norm.  With X the [K, D] matrix of flatten_weights (counters promoted to fp32):
 *   m     = torch.mean(X, dim=0)                           plato_agg_mean_rows
 *   cos_k = dot(x_k, m) / (|m| + 1e-9) / (|x_k| + 1e-9)    plato_agg_trust_stats, then
 *   w_k   = max(cos_k, 0) / (sum(max(cos, 0)) + 1e-9)      the host (plato_amd/trust.py)
 *   out   = sum_k x_k * w_k / |x_k + 1e-9| * |m|           plato_agg_scaled_sum
 *
 * plato_agg_trust_stats  <- torch.dot(weight, model_re), torch.norm(weight),
 *                           torch.norm(weight + 1e-9), torch.norm(model_re)
 *   With c_k[e] = x_k[e] in the fp32 region and (float)x_k[e] (round to nearest
 *   even) in the int64 region, and r[e] the reference vector (fp32 in both regions;
 *   for Fl-trust the output of plato_agg_mean_rows over the same table):
 *     d_out[k]      = sum over e of c_k[e] * r[e]
 *     d_out[K+k]    = sum over e of c_k[e]^2
 *     d_out[2K+k]   = sum over e of fp32(c_k[e] + eps)^2   (one fp32 addition)
 *     d_out[3K]     = sum over e of r[e]^2
 *   Every product is formed in float64 from its fp32 operands (exact: 24 + 24
 *   bits) and added in float64 in a fixed order: per lane over the coordinates of
 *   a chunk, across the lanes of a wave, across the waves of a workgroup, then
 *   over the chunks (through d_workspace, by a final kernel, in chunk order).  A
 *   region's chunk length is a multiple of PLATO_AGG_TRUST_TILE chosen by its
 *   coordinate count alone.  No atomics.
 *   Properties: (a) bitwise repeatable from run to run; (b) client k's three
 *   values depend only on row k, on r and on (n_f32, n_i64), not on K or on the
 *   order of the pointer table: a permuted table gives the bitwise permuted output;
 *   (c) each value is within D * 2^-53 * sum|terms| of the exact sum, D = n_f32 +
 *   n_i64; (d) NaN and +-inf propagate by IEEE rules.
 *   d_x_f32, d_x_i64   device arrays of K row pointers (d_x_i64 NULL when n_i64 == 0)
 *   d_ref_f32, d_ref_i64_as_f32  the reference vector's two regions, fp32
 *   d_workspace        plato_agg_trust_stats_workspace(K, n_f32, n_i64) bytes
 *                      (0: bad arguments), 256-byte aligned
 *   d_out              3K + 1 doubles, 16-byte aligned
 *   1 <= K <= PLATO_AGG_ROBUST_MAX_K; fewer than 2^38 coordinates per region;
 *   n_f32 == n_i64 == 0 is a success that launches nothing and writes nothing.
 *
 * plato_agg_scaled_sum  <- candidate = weight * w / torch.norm(weight + 1e-9) *
 *                          torch.norm(model_re); torch.sum(candidates, dim=0)
 *   for every coordinate e: acc = +0; for k = 0..K-1 in table order:
 *     t = c_k[e] * d_mul[k]; t = t / d_div[k] (IEEE division); t = t * post;
 *     acc = acc + t
 *   each operation fp32 and separately rounded, as ATen evaluates `x * w / n * nm`
 *   with 0-dim fp32 tensors.  No row is skipped: 0 * inf is NaN, as in the
 *   reference.  fp32 results for both regions.  d_mul and d_div are device arrays
 *   of K floats.  Same limits as plato_agg_mean_rows.
 *
 * Documented divergences from the reference, all by rounding or range only:
 *   - the mean and the final sum are sequential over the rows; ATen's torch.mean
 *     and torch.sum(dim=0) are blocked, equal to the sequential sum only for
 *     small K (any-order summation bound, as for plato_agg_mean_rows);
 *   - dots and norms are float64 sums; the reference's are fp32 (BLAS sdot and
 *     ATen's norm), whose own error grows with D;
 *   - the square root is taken in float64 (plato_amd/trust.py): a squared norm
 *     above the fp32 maximum gives a finite norm where the reference gives inf.
 */
#define PLATO_AGG_TRUST_TILE 1024
size_t plato_agg_trust_stats_workspace(int K, size_t n_f32, size_t n_i64);
int plato_agg_trust_stats(const float* const* d_x_f32, const int64_t* const* d_x_i64, int K,
                          const float* d_ref_f32, const float* d_ref_i64_as_f32, float eps,
                          size_t n_f32, size_t n_i64, void* d_workspace,
                          double* d_out /* 3K + 1 */, hipStream_t stream);
int plato_agg_scaled_sum(const float* const* d_x_f32, const int64_t* const* d_x_i64, int K,
                         const float* d_mul /* K */, const float* d_div /* K */, float post,
                         float* d_out_f32, float* d_out_i64_as_f32,
                         size_t n_f32, size_t n_i64, hipStream_t stream);

/*
 * Attack simulation (examples/detector/attacks.py, "LIE", "Lambda_attack", "Min-Max"
 * and "Min-Sum" of clients.attack_type): the attackers' rows get one poison vector
 * added in place.  With X the [A, D] matrix of flatten_weights over the attackers'
 * deltas (counters promoted to fp32) and W the same over their weights:
 *   LIE      poison = z * (-1 * torch.std(X, dim=0))           plato_agg_column_std
 *   Lambda   poison = lambada_value * (-1 * torch.mean(X, 0))  plato_agg_mean_rows
 *   Min-Max  poison = -1 * lam * p, p = avg / |avg|, avg = torch.mean(X, 0)
 *   Min-Sum  poison = lam * p,      p = avg / |avg|, avg = torch.mean(W, 0)
 * lam is found on the host (plato_amd/attacks.py) from plato_agg_pairwise_sqdist of
 * the delta rows and plato_agg_trust_stats of the delta rows against avg and p;
 * p is plato_agg_scale_by_norm(avg, fp32(|avg|), eps = 0): one fp32 division per
 * element, |avg| the float64 square root of the float64 sum of squares.
 *
 * plato_agg_column_std  <- torch.std(attacker_deltas, dim=0) (attacks.py:196)
 *   ATen's unbiased standard deviation: per coordinate e a sequential Welford update
 *   in float64 over the rows, in table order:
 *     mean = 0; m2 = 0
 *     for r = 0..m-1, x = (double)c_r[e]:
 *       d = x - mean; mean = mean + d / (double)(r + 1) (IEEE division);
 *       m2 = m2 + d * (x - mean)
 *     out[e] = (float)sqrt(m2 / (double)(m - 1))
 *   every operation float64 and separately rounded, c_r[e] = x_r[e] in the fp32
 *   region and (float)x_r[e] (round to nearest even) in the int64 region.  m == 1
 *   gives NaN (0 / 0), as torch does; identical rows give exactly +0; a NaN or an
 *   infinity stays in its own coordinate; values near FLT_MAX overflow to inf only
 *   at the final conversion.  fp32 results for both regions.  Equal to torch.std on
 *   the CPU bit for bit (it has no blocked order: every m).  1 <= m <= 256.
 *
 * plato_agg_add_scaled_rows  <- perform_model_poisoning (attacks.py:45-63)
 *   for every coordinate e: t = s * d_v[e] (one fp32 multiplication), then for every
 *   row r of the table, in place:
 *     fp32 region:   x_r[e] = x_r[e] + t                 (one fp32 addition)
 *     int64 region:  x_r[e] = x_r[e] + (int64)t          (truncation toward zero;
 *                    NaN and values outside [-2^63, 2^63) give INT64_MIN, as
 *                    plato_agg_cast_f32_i64; the addition wraps)
 *   The rows are distinct buffers; rows not in the table are not touched.  The
 *   attacks map onto (s, v) with the reference's own roundings, the exact negation
 *   folded into the scalar:
 *     LIE      s = -fp32(z),               v = std    (z * (-std) == (-z) * std)
 *     Lambda   s = -fp32(lambada_value),   v = mean
 *     Min-Max  s = -lam,                   v = p
 *     Min-Sum  s = lam,                    v = p
 *   d_v_f32, d_v_i64_as_f32: the vector's two regions, fp32, 4-byte aligned.
 *   Same limits as plato_agg_mean_rows.
 *
 * Documented divergences from the reference, all by rounding only:
 *   - torch.mean is blocked from m = 5 up; the mean here is the sequential row sum
 *     (plato_agg_mean_rows above);
 *   - the searches evaluate the reference's |u_k - avg + lam * p|^2 from float64 dots
 *     and squared norms of the fp32 vectors (no pass over the rows per step); the
 *     reference forms it in fp32.  Min-Sum's row sums of the distance matrix are
 *     float64, the reference's fp32;
 *   - |avg| is taken in float64 and rounded to fp32 once.
 */
int plato_agg_column_std(const float* const* d_x_f32, const int64_t* const* d_x_i64, int m,
                         float* d_out_f32, float* d_out_i64_as_f32,
                         size_t n_f32, size_t n_i64, hipStream_t stream);
int plato_agg_add_scaled_rows(float* const* d_x_f32, int64_t* const* d_x_i64, int m, float s,
                              const float* d_v_f32, const float* d_v_i64_as_f32,
                              size_t n_f32, size_t n_i64, hipStream_t stream);

/*
 * FLDetector (examples/detector/detectors.py:67-106 lbfgs, 310-418 fl_detector,
 * "FLDetector" of server.detector_type): the mean update of a round is predicted
 * from a record of N global-weight differences S and N mean-update differences Y by
 * the L-BFGS compact form, and every client is scored by the distance of its update
 * to the prediction.  The 2N x 2N system and the clustering of the K scores are the
 * host's (plato_amd/detectors.py); everything that streams the model is here.
 *
 * Notation.  D = n_f32 + n_i64.  A flat row is D contiguous fp32 values in arena
 * order: the fp32 region, then the int64 region as fp32; it is 4-byte aligned.
 * c_k[e] is client k's weight (x in the fp32 region, (float)x in the int64 region),
 * d_k[e] its delta as plato_agg_compute_deltas forms it, promoted to fp32: the fp32
 * subtraction x - b in the fp32 region, the wrapping int64 subtraction rounded once
 * to fp32 in the int64 region.  b is the baseline arena, bf[e] = b[e] or (float)b[e].
 *
 * plato_agg_detect_means  <- torch.mean(flattened_deltas_attacked, dim=0),
 *                            torch.mean(weights_attacked - last_weights, dim=0),
 *                            flattened_baseline_weights - last_weights,
 *                            mean - last_gradients
 *   One pass over the K client rows, b, last_w and last_g writes the four flat rows
 *   g, v, s_new, y_new, and the baseline as a flat row (the next round's last_w):
 *     g[e]     = (float)(sum_k (double)d_k[e] / (double)K)
 *     v[e]     = (float)(sum_k (double)fp32(c_k[e] - last_w[e]) / (double)K)
 *     s_new[e] = fp32(bf[e] - last_w[e])
 *     y_new[e] = fp32(g[e] - last_g[e])
 *     b_flat[e] = bf[e]
 *   The sums start at +0 and run over k in table order in float64, each addition
 *   and the division separately rounded; fp32(.) is one fp32 subtraction.
 *
 * plato_agg_rows_dots  <- torch.matmul(global_weights, gradients.T) and its kin
 *   d_out[r * m + j] = sum over e of rows[r][e] * vecs[j][e] for R flat rows and m
 *   flat vectors.  Every product is formed in float64 from its fp32 operands (exact)
 *   and added in plato_agg_trust_stats' fixed order, chunked by D alone.  Its
 *   properties (a)-(d) hold: repeatable; the value for (r, j) depends only on row r,
 *   vector j and D (and is the same bits with the two exchanged); within D * 2^-53 *
 *   sum|terms| of the exact sum; NaN and +-inf propagate.  Each row is read once per
 *   call, whatever m is.
 *   d_rows, d_vecs   device arrays of R and of m flat-row pointers
 *   d_workspace      plato_agg_rows_dots_workspace(R, m, D) bytes (0: bad arguments),
 *                    256-byte aligned
 *   d_out            R * m doubles, 16-byte aligned
 *   1 <= R <= PLATO_AGG_DETECT_MAX_ROWS; 1 <= m <= PLATO_AGG_DETECT_MAX_VECTORS.
 *
 * plato_agg_lbfgs_predict  <- last_gradients + (sigma * v - [sigma * S.T, Y.T] @ c)
 *   for every coordinate e: acc = +0; for j = 0..R-1 in table order:
 *     acc = acc + d_a[j] * (double)rows[j][e]
 *   pred[e] = (float)(((double)last_g[e] + sigma * (double)v[e]) - acc)
 *   every multiplication and addition float64 and separately rounded.  d_a is a
 *   device array of R doubles.
 *
 * plato_agg_delta_sqdist  <- torch.norm(pred_grad - flattened_deltas_attacked, dim=1)
 *   d_out[k] = sum over e of ((double)pred[e] - (double)d_k[e])^2: the float64
 *   difference and its square separately rounded, added in plato_agg_trust_stats'
 *   fixed order (the fp32 region's chunks, then the int64 region's) with the same
 *   four properties; client k's value depends only on row k, b, pred and
 *   (n_f32, n_i64).
 *   d_workspace      plato_agg_delta_sqdist_workspace(K, n_f32, n_i64) bytes
 *   d_out            K doubles, 16-byte aligned
 *
 * All four: 1 <= K <= PLATO_AGG_ROBUST_MAX_K; fewer than 2^38 coordinates; no
 * coordinates is a success that launches nothing and writes nothing.
 *
 * Documented divergences from the reference, all by rounding only: the means, the
 * dots, the prediction and the distances are float64 sums rounded once where the
 * reference's are fp32 (ATen's blocked sums, BLAS sgemm); the system is solved in
 * float64 on the host where the reference inverts it in fp32.
 */
#define PLATO_AGG_DETECT_MAX_ROWS 65536
#define PLATO_AGG_DETECT_MAX_VECTORS 4
int plato_agg_detect_means(const float* const* d_x_f32, const int64_t* const* d_x_i64, int K,
                           const float* d_b_f32, const int64_t* d_b_i64,
                           const float* d_last_w, const float* d_last_g, float* d_g, float* d_v,
                           float* d_s_new, float* d_y_new, float* d_b_flat,
                           size_t n_f32, size_t n_i64, hipStream_t stream);
size_t plato_agg_rows_dots_workspace(int R, int m, size_t D);
int plato_agg_rows_dots(const float* const* d_rows, int R, const float* const* d_vecs, int m, size_t D,
                        void* d_workspace, double* d_out /* R * m */, hipStream_t stream);
int plato_agg_lbfgs_predict(const float* const* d_rows, int R, const double* d_a /* R */, double sigma,
                            const float* d_last_g, const float* d_v, float* d_pred, size_t D,
                            hipStream_t stream);
size_t plato_agg_delta_sqdist_workspace(int K, size_t n_f32, size_t n_i64);
int plato_agg_delta_sqdist(const float* const* d_x_f32, const int64_t* const* d_x_i64, int K,
                           const float* d_b_f32, const int64_t* d_b_i64, const float* d_pred,
                           size_t n_f32, size_t n_i64, void* d_workspace, double* d_out /* K */,
                           hipStream_t stream);

/*
 * Global magnitude pruning (plato/processors/unstructured_pruning.py, the
 * "unstructured_pruning" outbound processor: torch.nn.utils.prune.global_unstructured
 * with L1Unstructured): of all prunable weights together, the k with the smallest
 * magnitude become zero.
 *
 * plato_agg_prune_global  <- torch.topk(|w|, k, largest=False) over the concatenated
 *                            weights, then w * mask
 *   works in place on one fp32 row of n_row elements.  The prunable elements are the
 *   pieces [begin, end) of h_pieces (elements of the row; `entry` is not read), taken
 *   in table order: that order is the flat index, and n their total count.  Pieces
 *   are ascending and disjoint; they may be empty and need not start on a 16-byte
 *   boundary.  Every element of the row outside the pieces keeps its bits.
 *
 *   key(w) = bits(w) & 0x7fffffff, compared as an unsigned integer: |w| in torch.topk's
 *   order, NaN largest.  T is the key of rank k - 1 (0-based) in the ascending order of
 *   the n keys.  An element is pruned if key < T; of the elements with key == T, the
 *   r = k - #(key < T) with the lowest flat indices are pruned (torch.topk's choice
 *   among them is unspecified).  Exactly k elements are pruned.  Only integer
 *   comparisons and integer sums decide: the result is the same bits on every run.
 *
 *   A pruned element becomes w * 0.0f as x86-64 evaluates it, formed from the bits:
 *   bits & 0x80000000 for a finite w (a negative weight gives -0.0), bits | 0x00400000
 *   for a NaN (quieted; sign and payload kept), 0xffc00000 for +-inf.  Every other
 *   element keeps its bits (the reference's w * 1.0f quiets a signalling NaN; this
 *   does not).
 *
 *   T is found by a radix select over the pieces in HBM, most significant digit first,
 *   in 3 passes (11, 10 and 10 bits); with the masked write and, only when
 *   0 < r < #(key == T), one more read that ranks the ties, the row is read 4 or 5
 *   times and written once.  All launches are ordered by `stream`; nothing returns to
 *   the host between them.
 *
 *   h_pieces     HOST table of n_pieces rows; it is uploaded on `stream` ahead of the
 *                kernels, so it stays unchanged until the stream reaches them
 *   d_workspace  plato_agg_prune_global_workspace(n_pieces, n) bytes (0: bad
 *                arguments), 256-byte aligned
 *   d_result     4 uint64, 16-byte aligned: T, #(key < T), #(key == T), r
 *   The table is checked before any GPU work (PLATO_AGG_EINVAL, message in
 *   plato_agg_last_error): a piece with end < begin, pieces that overlap or are out
 *   of order, a piece past n_row, k > n, more than 2^20 pieces, n_row >=
 *   2^32 (the counters and the piece table are 32-bit; n <= n_row).  k = 0 is a
 *   success that launches nothing and writes nothing, d_result included; k = n prunes
 *   every element.  d_row is 16-byte aligned.
 *
 *   A streaming launch has at most PLATO_AGG_PRUNE_GRID workgroups, each taking
 *   PLATO_AGG_PRUNE_TILE elements per grid step.
 */
#define PLATO_AGG_PRUNE_TILE 4096
#define PLATO_AGG_PRUNE_GRID 1024
#define PLATO_AGG_PRUNE_MAX_ELEMENTS 0xffffffffull
size_t plato_agg_prune_global_workspace(size_t n_pieces, size_t n_total);
int plato_agg_prune_global(float* d_row, size_t n_row, const plato_agg_chunk* h_pieces, size_t n_pieces, size_t k,
                           void* d_workspace, uint64_t* d_result /* 4 */, hipStream_t stream);

/*
 * QSGD quantizer (plato/processors/model_quantize_qsgd.py, the "model_quantize_qsgd"
 * outbound processor: Processor._process_layer): every entry of a state_dict becomes
 * its maximum magnitude and one byte per element, stochastically rounded to one of
 * `level` magnitudes.  plato_agg_fedavg_qsgd and plato_agg_decode_rows read these codes.
 *
 * plato_agg_qsgd_encode  <- max_v = max|layer|, level = ceil(|v| / max_v * (s - 1) - 1),
 *                           zeta = level + (random() <= |v| / max_v * (s - 1) - level),
 *                           the sign, one byte per value
 *   reads one fp32 row of n_row elements.  The entries are the pieces [begin, end) of
 *   h_pieces (elements of the row; `entry` is not read).  Pieces are ascending and
 *   disjoint; they may be empty and need not start on a 16-byte boundary.  d_codes[i] is
 *   the code of d_row[i]: every byte of d_codes outside the pieces keeps its value.
 *
 *   d_max_key[p] = max over piece p of bits(v) & 0x7fffffff, as an unsigned integer: the
 *   bits of m = max |v| when every value is finite.  0 marks an all-zero (or empty)
 *   piece, a key >= 0x7f800000 a piece that holds an infinity or a NaN.
 *
 *   With tp = (float)(level - 1), every operation a separately rounded fp32 operation
 *   (nothing is contracted to an fma):
 *     x    = (|v| / m) * tp                  IEEE division, subnormals kept
 *     lvl  = ceil(x - 1)                     -1 when x - 1 rounds to -1: then p = 1
 *     p    = x - lvl                         in (0, 1]
 *     mag  = lvl + (u <= p ? 1 : 0)          in [0, level - 1]
 *     code = mag | (0x80 if v < 0 and mag > 0)     -0.0 and a negative that rounds to 0
 *                                                  give 0x00, never 0x80
 *   u of row element i depends on (seed, i) alone, not on the pieces:
 *     h = splitmix64(key + (i >> 1)), key as plato_agg_fill_synth_* derives it from
 *         (seed, stream 0x51534744)
 *     u = (float)((i even ? h >> 40 : h >> 16) & 0xffffff) * 2^-24
 *   An all-zero piece gets zero codes (the reference fails on one).  A non-finite piece
 *   gets unspecified codes, inside the piece only.  Only integer maxima are reduced: the
 *   codes and the maxima are the same bytes on every run and for every grid.
 *
 *   The row is read twice and one byte per element is written.  All launches are
 *   ordered by `stream`; nothing returns to the host between them.
 *
 *   h_pieces     HOST table of n_pieces rows; it is uploaded on `stream` ahead of the
 *                kernels, so it stays unchanged until the stream reaches them
 *   d_codes      n_row bytes, 4-byte aligned
 *   d_max_key    n_pieces uint32
 *   d_workspace  plato_agg_qsgd_encode_workspace(n_pieces, n) bytes (0: bad arguments),
 *                256-byte aligned; n is the pieces' total count
 *   The arguments are checked before any GPU work (PLATO_AGG_EINVAL, message in
 *   plato_agg_last_error): a level outside [2, 128], a piece with end < begin, pieces
 *   that overlap or are out of order, a piece past n_row, more than 2^20 pieces, n_row
 *   >= 2^32, a null or misaligned pointer (d_row: 16 bytes).  n_pieces = 0 or n = 0 is
 *   a success that launches nothing and writes nothing, d_max_key included.
 *
 *   A streaming launch has at most PLATO_AGG_QSGD_ENCODE_GRID workgroups, each taking
 *   PLATO_AGG_QSGD_ENCODE_TILE elements per grid step.
 */
#define PLATO_AGG_QSGD_ENCODE_TILE 4096
#define PLATO_AGG_QSGD_ENCODE_GRID 1024
size_t plato_agg_qsgd_encode_workspace(size_t n_pieces, size_t n_total);
int plato_agg_qsgd_encode(const float* d_row, size_t n_row, const plato_agg_chunk* h_pieces, size_t n_pieces,
                          int level, uint64_t seed, uint8_t* d_codes /* n_row */, uint32_t* d_max_key /* n_pieces */,
                          void* d_workspace, hipStream_t stream);

/*
 * Sub-model aggregation (examples/model_search/{heterofl,fjord,fedrolex,anycostfl}:
 * Algorithm.aggregation): every client sends leading-corner boxes
 * value[:s0, :s1, ...] of the global tensors, and every global element becomes the
 * mean of the clients whose box covers it.
 *
 * plato_agg_submodel_mean  <- global[key][:s0, :s1, ...] += local[key] per client,
 *                             count likewise, torch.div(global[key] - value, count)
 *   for every element of every entry, with g its value in d_global:
 *     acc = g; count = 0
 *     for k = 0..K-1 in table order, if client k's box covers the element:
 *       acc = acc + x_k (fp32, separately rounded); count = count + 1
 *     out = (acc - g) / (float)max(count, 1)      (fp32 subtraction, IEEE division)
 *   An element no client covers is (g - g) / 1: +0 for a finite g, NaN for an
 *   infinite or NaN g.  g takes part in the rounding of every partial sum, and the
 *   table order is the order of the sum, as in the reference.
 *
 *   An entry is a run of d_global / d_out seen as [P, Q, L] (row-major); client k's
 *   box is (p <= P, q <= Q, l <= L) and covers the (i, j, t) with i < p, j < q,
 *   t < l; its value is d_rows[k][src + (i * q + j) * l + t] (64-bit arithmetic).
 *     a [D0] entry                [1, 1, D0]         box (1, 1, s0)
 *     a [D0, D1, R...] entry      [D0, 1, D1 * R]    box (s0, 1, s1 * R)
 *     a [D0, D1, D2] entry        [D0, D1, D2]       box (s0, s1, s2)
 *   h_entries  n_entries rows of PLATO_AGG_SUBMODEL_ENTRY_WORDS int64:
 *              {offset in d_global and d_out, P, Q, L, first tile, 0}, by ascending
 *              offset and not overlapping; the first tile of an entry is the sum of
 *              ceil(P * Q * L / PLATO_AGG_SUBMODEL_TILE) over the entries before it.
 *              Elements of d_out that no entry holds are not written.
 *   h_boxes    n_entries * K rows of PLATO_AGG_SUBMODEL_BOX_WORDS int64, entry-major:
 *              {p, q, l, src}.  src == PLATO_AGG_SUBMODEL_ABSENT with zero extents:
 *              the client has no box of this entry (an extent of 0 covers nothing
 *              either).  Boxes in four dims, with keys that a client lacks, are
 *              plato_agg_elastic_mean's below, under tables of its own.
 *   h_row_len  K int64: the elements of each client row, for the bounds check
 *   d_rows     device array of K row pointers (4-byte aligned rows)
 *   d_tables   plato_agg_submodel_tables_bytes(K, n_entries) bytes (0: bad
 *              arguments), 256-byte aligned: the call copies both tables there on
 *              `stream` ahead of the kernel, so the host tables stay unchanged until
 *              the stream has passed the call
 *   d_out      n_out floats, 16-byte aligned
 *   The three host tables are checked before any GPU work: extents and offsets in
 *   range, no box above its entry's extents or past its client's row length.
 *   1 <= K <= PLATO_AGG_SUBMODEL_MAX_K; at most 2^20 entries; fewer than 2^38
 *   elements; n_entries == 0 or n_out == 0 is a success that launches nothing.
 *   Bitwise repeatable; no atomics.
 */
#define PLATO_AGG_SUBMODEL_MAX_K 4096
#define PLATO_AGG_SUBMODEL_MAX_ENTRIES 1048576
#define PLATO_AGG_SUBMODEL_TILE 1024
#define PLATO_AGG_SUBMODEL_ENTRY_WORDS 6
#define PLATO_AGG_SUBMODEL_BOX_WORDS 4
#define PLATO_AGG_SUBMODEL_ABSENT (-1)
size_t plato_agg_submodel_tables_bytes(int K, size_t n_entries);
int plato_agg_submodel_mean(const float* d_global, const float* const* d_rows, int K,
                            const int64_t* h_row_len /* K */, const int64_t* h_entries, const int64_t* h_boxes,
                            size_t n_entries, void* d_tables, float* d_out, size_t n_out, hipStream_t stream);

/*
 * Elastic sub-model aggregation (examples/model_search/sysheterofl: Algorithm.aggregation,
 * sysheterofl_algorithm.py:134-181): the clients differ in depth, so a client lacks
 * whole keys of the global model, and in width per stage; a 4-D tensor is boxed on
 * all four dims, and every key takes part, running statistics included.
 *
 * The rule, with G = algorithm.model.state_dict() and the clients in arrival order;
 * update_track is a bool (default true).  For every key of G, in G's order:
 *   rank      by G[key].dim(): 4 -> 4, 2 -> 2, 1 -> 1, any other dim -> 0; with
 *             update_track false a 1-D key whose name contains "running" or "tracked"
 *             has rank 0.
 *   a client  takes part in a key only if the key is in its payload and the rank is at
 *             least 1.  Its tensor is float32, has as many dims as G[key] and no extent
 *             above G[key]'s, and covers the leading-corner box [:s0, :s1, :s2, :s3]
 *             ([:s0, :s1]; [:s0]).  An extent of 0 covers nothing.  Keys of the
 *             payload that G lacks are ignored; keys of rank 0 are never read.
 *   element   acc = g; acc = acc + x_k over the clients that hold the key and cover
 *             the element, in arrival order; out = (acc - g) / max(count, 1): every
 *             operation a separately rounded fp32 one, the division IEEE.  An element
 *             nobody covers (a whole entry no client of the round holds included) is
 *             (g - g) / 1: +0 for a finite g (also for -0), NaN for an infinite or
 *             NaN g.
 *   result    float32 for every key.  A key of G that is not float32 gives float32
 *             zeros of its shape if its dtype is an integer one and its dim is not 1,
 *             2 or 4 (the 0-D int64 num_batches_tracked counters: an int64 g - g is
 *             exactly 0), written by the caller without GPU work; any other
 *             non-float32 key of G is refused by the caller.
 *
 * plato_agg_elastic_mean computes the float32 keys.
 *   An entry is a run of d_global / d_out seen row-major as [A, B, C, D]; a box
 *   (a <= A, b <= B, c <= C, d <= D) covers the (i, j, t, u) with i < a, j < b, t < c,
 *   u < d, and its value is d_rows[client][src + ((i * b + j) * c + t) * d + u]
 *   (64-bit arithmetic).  Trailing dims in which every holder has the full extent
 *   may be merged into the dim before them (a convolution whose holders all have
 *   the global kernel size is [1, 1, D0, D1 * kh * kw], boxes (1, 1, s0, s1 * kh * kw));
 *   the kernel pays an integer division only for view dims whose extent is not 1.
 *   h_entries  n_entries rows of PLATO_AGG_ELASTIC_ENTRY_WORDS int64:
 *              {offset in d_global and d_out, A, B, C, D, first tile, first box,
 *              number of boxes}, by ascending offset and not overlapping.  The first
 *              tile of an entry is the sum of ceil(A * B * C * D /
 *              PLATO_AGG_ELASTIC_TILE) over the entries before it, its first box the
 *              sum of their numbers of boxes; the box ranges tile [0, n_boxes).
 *              Elements of d_out that no entry holds are not written.
 *   h_boxes    n_boxes rows of PLATO_AGG_ELASTIC_BOX_WORDS int64: {a, b, c, d, src,
 *              client}.  The table is compact: an entry lists the clients that hold
 *              it and no others, by strictly ascending client (0 <= client < K), so
 *              the arrival order is the order of the sum; an entry nobody holds has
 *              zero boxes, and there is no absent encoding.
 *   h_row_len  K int64: the elements of each client row (0 is legal: the client holds
 *              no key), for the bounds check src + a * b * c * d <= h_row_len[client]
 *   d_rows     device array of K row pointers (4-byte aligned rows)
 *   d_tables   plato_agg_elastic_tables_bytes(n_entries, n_boxes) bytes (0: bad
 *              arguments), 256-byte aligned: the call copies both tables there on
 *              `stream` ahead of the kernel, so the host tables stay unchanged until
 *              the stream has passed the call
 *   d_out      n_out floats, 16-byte aligned
 *   The three host tables are checked before any GPU work (negative status,
 *   plato_agg_last_error): K, the entries' ranges, the tile column, the box ranges,
 *   the clients' order, the extents, the row lengths.
 *   1 <= K <= PLATO_AGG_ELASTIC_MAX_K; at most 2^20 entries and 2^20 * K boxes;
 *   fewer than 2^38 elements; n_entries == 0 or n_out == 0 is a success that launches
 *   nothing.  Nothing is sized by K.  Bitwise repeatable; no atomics.
 */
#define PLATO_AGG_ELASTIC_MAX_K 4096
#define PLATO_AGG_ELASTIC_MAX_ENTRIES 1048576
#define PLATO_AGG_ELASTIC_TILE 1024
#define PLATO_AGG_ELASTIC_ENTRY_WORDS 8
#define PLATO_AGG_ELASTIC_BOX_WORDS 6
size_t plato_agg_elastic_tables_bytes(size_t n_entries, size_t n_boxes);
int plato_agg_elastic_mean(const float* d_global, const float* const* d_rows, int K,
                           const int64_t* h_row_len /* K */, const int64_t* h_entries, size_t n_entries,
                           const int64_t* h_boxes, size_t n_boxes, void* d_tables,
                           float* d_out, size_t n_out, hipStream_t stream);

/*
 * Single-process RCCL communicator over the GPUs one Plato server drives.
 * The reference has no collectives (aggregation runs on one CPU
 * process); these serve the multi-GPU engine behind the same
 * aggregate_weights hook (plato/servers/fedavg.py:171-182), which bucket-
 * shards the arena over the node's GPUs.  Rank g is
 * devices[g]; every collective is issued for all ranks inside one
 * ncclGroupStart/End, each on its own stream (streams[g] on devices[g]).
 * RCCL is bound at run time (dlopen "librccl.so.1"): PLATO_AGG_ERCCL if absent.
 */
typedef struct plato_agg_comm plato_agg_comm;

/* ncclCommInitAll over `ndev` distinct device ordinals. */
int plato_agg_comm_create(int ndev, const int* devices, plato_agg_comm** out);
int plato_agg_comm_destroy(plato_agg_comm* comm);
int plato_agg_comm_size(const plato_agg_comm* comm);

/* d_recv[g][r*count .. (r+1)*count) = d_send[r][0 .. count) for every rank r:
 * assembles the bucket-sharded new model on every GPU. */
int plato_agg_comm_allgather_f32(plato_agg_comm* comm, const float* const* d_send, float* const* d_recv,
                                 size_t count, const hipStream_t* streams);

/* d_recv[g][0 .. count) = sum over ranks r of d_send[r][g*count .. (g+1)*count)
 * (client-sharded tolerance mode: per-GPU partial weighted sums -> bucket g). */
int plato_agg_comm_reduce_scatter_f32(plato_agg_comm* comm, const float* const* d_send, float* const* d_recv,
                                      size_t count, const hipStream_t* streams);

#ifdef __cplusplus
}
#endif

#endif /* PLATO_AGG_H */
