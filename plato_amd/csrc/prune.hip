// prune.hip — gfx950 kernels for global magnitude pruning, the reference's outbound processor
// `unstructured_pruning` (plato/processors/unstructured_pruning.py: torch.nn.utils.prune.global_unstructured
// with L1Unstructured), exported through the C ABI in include/plato_agg.h as plato_agg_prune_global.
//
// Design ("Global magnitude pruning"):
//  * The key of a weight is bits & 0x7fffffff: |w| in the order torch.topk ranks it (NaN largest), as an
//    unsigned integer.  The threshold T is the key of rank k - 1; it is found by a radix select, most
//    significant digit first, in three passes of 11, 10 and 10 bits (bit 31 of a key is 0).  A pass is a
//    streaming read of the pieces: every workgroup counts the digits of the keys that match the prefix found
//    so far in an LDS histogram and adds its non-empty bins to one global histogram; a one-workgroup kernel
//    then scans the histogram, fixes the digit and the rank that remains.  Integer adds only: the histogram
//    does not depend on the order in which they land.
//  * The prunable elements are tiled per piece (pieces.h, shared with qsgd_encode.hip): a tile wholly inside
//    its piece is read and written with 16-byte accesses; the first and last tile of a piece take a guarded
//    path that touches nothing outside [b, e).  Tile order is flat-index order.
//  * The apply pass prunes key < T, and of the elements with key == T the r = k - #(key < T) with the lowest
//    flat indices.  Only when 0 < r < #(key == T) does that need a ranking: one more read counts the ties of
//    every tile, a one-workgroup exclusive scan turns the counts into each tile's first tie rank, and the
//    apply pass ranks the ties inside its tile with a workgroup scan.  Both kernels leave at once otherwise.
//  * A pruned weight becomes w * 0.0f as the host the reference runs on evaluates it (x86-64 SSE), formed
//    from the bits: the sign alone for a finite w, the quieted NaN for a NaN, 0xffc00000 for an infinity.
//    Every other element keeps its bits.
//  * The launches are ordered by the stream alone; nothing comes back to the host between them.
#include "pieces.h"

namespace {

constexpr int kPasses = 3;
constexpr int kMaxBins = 2048;
__host__ __device__ constexpr int digit_bits(int pass) { return pass == 0 ? 11 : 10; }
__host__ __device__ constexpr int digit_shift(int pass) { return pass == 0 ? 20 : pass == 1 ? 10 : 0; }

// The head of the workspace.  Everything up to and including the tie counts is zeroed before the first launch.
struct Ctrl {
  uint32_t prefix;  // the digits fixed so far
  uint32_t rank;    // the rank that remains among the keys with that prefix
  uint32_t T, less, ties, r;
  uint32_t need_rank;  // 0 < r < ties
  uint32_t pad[57];
  uint32_t hist[kPasses][kMaxBins];
};
static_assert(sizeof(Ctrl) == 256 + kPasses * kMaxBins * 4, "Ctrl is the 256-byte head and the histograms");

// w * 0.0f as x86-64 SSE evaluates it, from the bits of w
__device__ __forceinline__ uint32_t times_zero(uint32_t bits) {
  const uint32_t key = key_of(bits);
  if (key > 0x7f800000u) return bits | 0x00400000u;  // NaN: quieted, sign and payload kept
  if (key == 0x7f800000u) return 0xffc00000u;        // inf * 0: the default NaN
  return bits & 0x80000000u;
}

// ------------------------------------------------------------------ one digit's histogram
template <int kPass>
__global__ __launch_bounds__(kThreads) void hist_kernel(const uint32_t* __restrict__ row, Tiles tl, Ctrl* ctrl) {
  constexpr int kBins = 1 << digit_bits(kPass);
  constexpr int kShift = digit_shift(kPass);
  __shared__ uint32_t h[kBins];
  for (int i = threadIdx.x; i < kBins; i += kThreads) h[i] = 0;
  const uint32_t prefix = kPass ? sld(&ctrl->prefix, 0) : 0;
  __syncthreads();
  // A lane holds back its last digit and the number of times it came in a row, and adds when another digit
  // follows: a run of equal keys (the zeros of a pruned model, which match the prefix in every pass) is one
  // add, not a pile-up on one address.  Keys that differ from their neighbours still cost an add each.
  uint32_t held = 0, run = 0;
  for (uint32_t t = blockIdx.x; t < tl.n_tiles; t += gridDim.x) {
    Share sh;
    load_tile(row, tl, t, sh);
#pragma unroll
    for (int s = 0; s < kSlots; ++s)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const uint32_t key = key_of(sh.bits[s][c]);
        const bool counts = (sh.valid[s] >> c & 1) && (kPass == 0 || (key >> (kShift + digit_bits(kPass))) == prefix);
        if (counts) {
          const uint32_t digit = (key >> kShift) & (kBins - 1);
          if (run && digit != held) {
            atomicAdd(&h[held], run);
            run = 0;
          }
          held = digit;
          ++run;
        }
      }
  }
  if (run) atomicAdd(&h[held], run);
  __syncthreads();
  for (int i = threadIdx.x; i < kBins; i += kThreads)
    if (h[i]) atomicAdd(&ctrl->hist[kPass][i], h[i]);
}

// ------------------------------------------------------------------ the digit that holds the rank
// One workgroup.  rank0: the rank sought by the first pass (k - 1).  The last pass writes the record.
template <int kPass>
__global__ __launch_bounds__(kThreads) void pick_kernel(Ctrl* ctrl, uint32_t rank0, uint64_t k, uint64_t* d_result) {
  constexpr int kBins = 1 << digit_bits(kPass);
  constexpr int kPer = kBins / kThreads;
  __shared__ uint32_t wt[kWaves];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t prefix = kPass ? ctrl->prefix : 0;
  const uint32_t rank = kPass ? ctrl->rank : rank0;
  uint32_t c[kPer], sum = 0;
#pragma unroll
  for (int i = 0; i < kPer; ++i) sum += c[i] = ctrl->hist[kPass][threadIdx.x * kPer + i];
  const uint32_t incl = wave_inclusive(sum);
  if (lane == 63) wt[wave] = incl;
  __syncthreads();  // also orders the reads of prefix and rank above before the writes below
  uint32_t below = incl - sum;
  for (uint32_t w = 0; w < wave; ++w) below += wt[w];
  // the counts of the bins add up to more than rank, so exactly one lane's bins hold it
  if (rank < below || rank - below >= sum) return;
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    if (rank - below < c[i]) {
      const uint32_t now = (prefix << digit_bits(kPass)) | (threadIdx.x * kPer + i);
      const uint32_t left = rank - below;
      ctrl->prefix = now;
      ctrl->rank = left;
      if (kPass == kPasses - 1) {
        const uint32_t r = left + 1, less = uint32_t(k - r), ties = c[i];
        ctrl->T = now;
        ctrl->less = less;
        ctrl->ties = ties;
        ctrl->r = r;
        ctrl->need_rank = r < ties;
        d_result[0] = now;
        d_result[1] = less;
        d_result[2] = ties;
        d_result[3] = r;
      }
      return;
    }
    below += c[i];
  }
}

// ------------------------------------------------------------------ the ties of every tile
__global__ __launch_bounds__(kThreads) void tie_count_kernel(const uint32_t* __restrict__ row, Tiles tl,
                                                            const Ctrl* __restrict__ ctrl,
                                                            uint32_t* __restrict__ tile_ties) {
  if (!sld(&ctrl->need_rank, 0)) return;
  const uint32_t T = sld(&ctrl->T, 0);
  for (uint32_t t = blockIdx.x; t < tl.n_tiles; t += gridDim.x) {
    Share sh;
    load_tile(row, tl, t, sh);
    uint32_t n = 0;
#pragma unroll
    for (int s = 0; s < kSlots; ++s)
#pragma unroll
      for (int c = 0; c < 4; ++c) n += (sh.valid[s] >> c & 1) && key_of(sh.bits[s][c]) == T;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) n += __shfl_xor(n, off, 64);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&tile_ties[t], n);
  }
}

// ------------------------------------------------------------------ the masked write
// tile_first[t]: the rank among all ties of tile t's first tie (read only when 0 < r < ties).
__global__ __launch_bounds__(kThreads) void apply_kernel(uint32_t* __restrict__ row, Tiles tl,
                                                        const Ctrl* __restrict__ ctrl,
                                                        const uint32_t* __restrict__ tile_first) {
  __shared__ uint64_t wt[2][kWaves];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t T = sld(&ctrl->T, 0), r = sld(&ctrl->r, 0);
  const bool need_rank = sld(&ctrl->need_rank, 0) != 0;
  uint32_t it = 0;
  for (uint32_t t = blockIdx.x; t < tl.n_tiles; t += gridDim.x, ++it) {
    Share sh;
    load_tile(row, tl, t, sh);
    // rank[s]: the rank among all ties of the first tie in slot s of this lane; r ties are pruned.  A tile's
    // flat order is slot-major, then lane, then element: the four slots' counts are scanned over the lanes
    // at once, 16 bits each (a slot row holds at most 1024 ties).
    uint32_t rank[kSlots] = {0, 0, 0, 0};
    if (need_rank) {
      uint64_t mine = 0;
#pragma unroll
      for (int s = 0; s < kSlots; ++s) {
        uint32_t n = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) n += (sh.valid[s] >> c & 1) && key_of(sh.bits[s][c]) == T;
        mine |= uint64_t(n) << (16 * s);
      }
      const uint64_t incl = wave_inclusive(mine);
      if (lane == 63) wt[it & 1][wave] = incl;
      __syncthreads();  // one barrier a tile: the next tile writes the other buffer
      uint64_t before = incl - mine, all = 0;
#pragma unroll
      for (uint32_t w = 0; w < kWaves; ++w) {
        const uint64_t v = wt[it & 1][w];
        before += w < wave ? v : 0;
        all += v;
      }
      uint32_t first = tile_first[t];
#pragma unroll
      for (int s = 0; s < kSlots; ++s) {
        rank[s] = first + uint32_t(before >> (16 * s) & 0xffff);
        first += uint32_t(all >> (16 * s) & 0xffff);
      }
    }
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
      u32x4 out = sh.bits[s];
      uint32_t tie_rank = rank[s];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const uint32_t key = key_of(sh.bits[s][c]);
        const bool in = sh.valid[s] >> c & 1;
        bool prune = in && key < T;
        if (in && key == T) prune = tie_rank++ < r;  // without ranking every rank is 0 < r: all ties go
        if (prune) out[c] = times_zero(sh.bits[s][c]);
      }
      if (sh.full) {
        *(u32x4*)(row + sh.at[s]) = out;
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (sh.valid[s] >> c & 1) row[sh.at[s] + c] = out[c];
      }
    }
  }
}

// tiles of n_total elements in n_pieces pieces, at most: a piece of len elements has at most len / W + 2
inline uint64_t max_tiles(uint64_t n_pieces, uint64_t n_total) { return n_total / kTile + 2 * n_pieces; }

}  // namespace

extern "C" {

size_t plato_agg_prune_global_workspace(size_t n_pieces, size_t n_total) {
  if (n_pieces > kMaxPieces || n_total > PLATO_AGG_PRUNE_MAX_ELEMENTS) return 0;
  return sizeof(Ctrl) + round_up(max_tiles(n_pieces, n_total) * 4, 256) + round_up(n_pieces * 4, 256) +
         round_up(n_pieces * sizeof(plato_agg_chunk), 256);
}

int plato_agg_prune_global(float* d_row, size_t n_row, const plato_agg_chunk* h_pieces, size_t n_pieces, size_t k,
                           void* d_workspace, uint64_t* d_result, hipStream_t stream) {
  Plan plan;
  const char* why = first_refusal({
      n_pieces > kMaxPieces ? "more than 2^20 pieces" : nullptr,
      n_row > PLATO_AGG_PRUNE_MAX_ELEMENTS ? "the row has 2^32 elements or more" : nullptr,
      n_pieces && !h_pieces ? "null piece table" : nullptr,
  });
  if (!why) why = bad_pieces(h_pieces, n_pieces, n_row, &plan);
  if (!why && k > plan.n_total) why = "k exceeds the number of prunable elements";
  if (!why && k)
    why = first_refusal({
        !d_row || !d_workspace || !d_result ? "null row, workspace or result pointer" : nullptr,
        !aligned(d_row, 16) ? "the row must be 16-byte aligned" : nullptr,
        !aligned(d_workspace, 256) ? "workspace must be 256-byte aligned" : nullptr,
        !aligned(d_result, 16) ? "the result must be 16-byte aligned" : nullptr,
    });
  if (why) return fail(PLATO_AGG_EINVAL, why);
  if (!k) return plato_agg_internal::clear_error();

  // the workspace: Ctrl, the tiles' tie counts (both zeroed here), the pieces' first tiles, the piece table
  char* ws = static_cast<char*>(d_workspace);
  Ctrl* ctrl = reinterpret_cast<Ctrl*>(ws);
  uint32_t* tile_ties = reinterpret_cast<uint32_t*>(ws + sizeof(Ctrl));
  char* after = ws + sizeof(Ctrl) + round_up(max_tiles(n_pieces, plan.n_total) * 4, 256);
  uint32_t* first_tile = reinterpret_cast<uint32_t*>(after);
  plato_agg_chunk* d_pieces = reinterpret_cast<plato_agg_chunk*>(after + round_up(n_pieces * 4, 256));

  hipError_t err = hipMemsetAsync(ws, 0, sizeof(Ctrl) + round_up(plan.n_tiles * 4, 16), stream);
  if (err == hipSuccess)
    err = hipMemcpyAsync(d_pieces, h_pieces, n_pieces * sizeof(plato_agg_chunk), hipMemcpyHostToDevice, stream);
  if (err != hipSuccess) return fail(PLATO_AGG_EHIP, std::string("prune_global tables: ") + hipGetErrorString(err));

  const Tiles tl = {d_pieces, first_tile, uint32_t(n_pieces), uint32_t(plan.n_tiles)};
  const uint32_t* row_bits = reinterpret_cast<const uint32_t*>(d_row);
  const dim3 grid(uint32_t(plan.n_tiles < kGrid ? plan.n_tiles : kGrid)), block(kThreads), one(1);
  const uint32_t rank0 = uint32_t(k - 1);
  const uint64_t k64 = k;
  hipLaunchKernelGGL(scan_kernel<true>, one, block, 0, stream, first_tile, uint32_t(n_pieces), d_pieces, nullptr);
  hipLaunchKernelGGL(hist_kernel<0>, grid, block, 0, stream, row_bits, tl, ctrl);
  hipLaunchKernelGGL(pick_kernel<0>, one, block, 0, stream, ctrl, rank0, k64, d_result);
  hipLaunchKernelGGL(hist_kernel<1>, grid, block, 0, stream, row_bits, tl, ctrl);
  hipLaunchKernelGGL(pick_kernel<1>, one, block, 0, stream, ctrl, rank0, k64, d_result);
  hipLaunchKernelGGL(hist_kernel<2>, grid, block, 0, stream, row_bits, tl, ctrl);
  hipLaunchKernelGGL(pick_kernel<2>, one, block, 0, stream, ctrl, rank0, k64, d_result);
  hipLaunchKernelGGL(tie_count_kernel, grid, block, 0, stream, row_bits, tl, ctrl, tile_ties);
  hipLaunchKernelGGL(scan_kernel<false>, one, block, 0, stream, tile_ties, uint32_t(plan.n_tiles), nullptr,
                     &ctrl->need_rank);
  hipLaunchKernelGGL(apply_kernel, grid, block, 0, stream, reinterpret_cast<uint32_t*>(d_row), tl, ctrl, tile_ties);
  err = hipGetLastError();
  if (err != hipSuccess) return fail(PLATO_AGG_EHIP, std::string("prune_global: ") + hipGetErrorString(err));
  return plato_agg_internal::clear_error();
}

}  // extern "C"
