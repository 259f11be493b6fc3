// qsgd_encode.hip — gfx950 kernels for the QSGD quantizer, the reference's outbound processor
// `model_quantize_qsgd` (plato/processors/model_quantize_qsgd.py: Processor._process_layer), exported through
// the C ABI in include/plato_agg.h as plato_agg_qsgd_encode.  The decoder of these codes is qsgd.hip.
//
// Design ("QSGD quantizer"):
//  * The entries of a state_dict are the pieces of one fp32 device row, walked in tiles as prune.hip walks
//    them (pieces.h).
//  * Pass 1: the maximum per piece of key = bits & 0x7fffffff as an unsigned integer, which is max |v| for
//    finite values.  A lane keeps the maximum of its share while the piece stays the same; when the piece
//    changes the workgroup reduces (wave shuffles, then LDS) and issues one atomicMax.  Integers only: the
//    result does not depend on the order.  Key 0 is an all-zero piece, key >= 0x7f800000 a non-finite one.
//  * Pass 2: per element, with m the piece's maximum and tp = float(level - 1), each operation rounded to fp32
//    on its own (the library is built with -ffp-contract=off):
//        x = (|v| / m) * tp;  lvl = ceil(x - 1);  p = x - lvl;  mag = lvl + (u <= p);
//        byte = mag | (0x80 if v < 0 and mag > 0)
//    u of row element i is 24 bits of splitmix64(key + (i >> 1)): bits 40..63 for an even i, 16..39 for an
//    odd one, times 2^-24.  It depends on (seed, i) alone, so neither the grid nor the pieces around an
//    element change its code.
//  * A tile wholly inside its piece stores the four codes of a 16-byte slot as one dword.  A guarded tile
//    stores single bytes: two pieces may share a dword of the codes and are written by different workgroups.
//  * The launches are ordered by the stream alone; nothing comes back to the host between them.
#include "pieces.h"

namespace {

static_assert(PLATO_AGG_QSGD_ENCODE_TILE == PLATO_AGG_PRUNE_TILE && PLATO_AGG_QSGD_ENCODE_GRID == PLATO_AGG_PRUNE_GRID,
              "both walk the pieces with pieces.h");

constexpr uint64_t kDrawStream = 0x51534744;  // "QSGD"

// the counter generator of fedavg_agg.hip (oracle/synth.py)
__host__ __device__ inline uint64_t splitmix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
inline uint64_t synth_key(uint64_t seed, uint64_t stream_id) {
  return splitmix64(seed ^ (stream_id * 0xD1B54A32D192ED03ull));
}

__device__ __forceinline__ uint32_t wave_max(uint32_t x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const uint32_t y = __shfl_xor(x, off, 64);
    x = y > x ? y : x;
  }
  return x;
}

// ------------------------------------------------------------------ pass 1: max key per piece
// max_key is zeroed before the launch.
__global__ __launch_bounds__(kThreads) void max_kernel(const uint32_t* __restrict__ row, Tiles tl,
                                                      uint32_t* __restrict__ max_key) {
  __shared__ uint32_t wm[kWaves];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t mine = 0, piece = 0;
  bool open = false;
  // the piece is uniform, so every lane of the workgroup takes the same path to the barriers
  auto flush = [&]() {
    const uint32_t w = wave_max(mine);
    if (lane == 0) wm[wave] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t all = wm[0];
#pragma unroll
      for (int i = 1; i < kWaves; ++i) all = wm[i] > all ? wm[i] : all;
      if (all) atomicMax(&max_key[piece], all);
    }
    __syncthreads();  // wm is free again
    mine = 0;
  };
  for (uint32_t t = blockIdx.x; t < tl.n_tiles; t += gridDim.x) {
    Share sh;
    load_tile(row, tl, t, sh);
    if (open && sh.piece != piece) flush();
    piece = sh.piece;
    open = true;
#pragma unroll
    for (int s = 0; s < kSlots; ++s)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const uint32_t key = key_of(sh.bits[s][c]);  // an element outside the piece was loaded as 0
        mine = key > mine ? key : mine;
      }
  }
  if (open) flush();
}

// ------------------------------------------------------------------ pass 2: the codes
__device__ __forceinline__ uint32_t code_of(uint32_t bits, float m, float tp, float u) {
  const float ratio = __uint_as_float(key_of(bits)) / m;  // IEEE division, subnormals kept
  const float x = ratio * tp;
  const float lvl = ceilf(x - 1.0f);  // -1 for x <= 2^-25: then p = 1 and the magnitude is 0
  const float p = x - lvl;
  const uint32_t mag = uint32_t(int(lvl) + int(u <= p));
  return mag | ((bits >> 31) && mag ? 0x80u : 0u);
}

__global__ __launch_bounds__(kThreads) void encode_kernel(const uint32_t* __restrict__ row, Tiles tl,
                                                         const uint32_t* __restrict__ max_key, float tp,
                                                         uint64_t draw_key, uint8_t* __restrict__ codes) {
  for (uint32_t t = blockIdx.x; t < tl.n_tiles; t += gridDim.x) {
    Share sh;
    load_tile(row, tl, t, sh);
    const uint32_t mk = sld(max_key, int(sh.piece));
    const float m = __uint_as_float(mk);
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
      // at[s] is a multiple of 4: elements at[s] + 0..1 share one hash, at[s] + 2..3 the next
      const uint64_t h0 = splitmix64(draw_key + (sh.at[s] >> 1));
      const uint64_t h1 = splitmix64(draw_key + (sh.at[s] >> 1) + 1);
      const float u[4] = {float(uint32_t(h0 >> 40) & 0xffffffu) * 0x1p-24f, float(uint32_t(h0 >> 16) & 0xffffffu) * 0x1p-24f,
                          float(uint32_t(h1 >> 40) & 0xffffffu) * 0x1p-24f, float(uint32_t(h1 >> 16) & 0xffffffu) * 0x1p-24f};
      uint32_t code[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) code[c] = mk ? code_of(sh.bits[s][c], m, tp, u[c]) : 0u;  // an all-zero piece
      if (sh.full) {
        *reinterpret_cast<uint32_t*>(codes + sh.at[s]) = code[0] | code[1] << 8 | code[2] << 16 | code[3] << 24;
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (sh.valid[s] >> c & 1) codes[sh.at[s] + c] = uint8_t(code[c]);
      }
    }
  }
}

}  // namespace

extern "C" {

size_t plato_agg_qsgd_encode_workspace(size_t n_pieces, size_t n_total) {
  if (n_pieces > kMaxPieces || n_total > PLATO_AGG_PRUNE_MAX_ELEMENTS) return 0;
  return 256 + round_up(n_pieces * 4, 256) + round_up(n_pieces * sizeof(plato_agg_chunk), 256);
}

int plato_agg_qsgd_encode(const float* d_row, size_t n_row, const plato_agg_chunk* h_pieces, size_t n_pieces,
                          int level, uint64_t seed, uint8_t* d_codes, uint32_t* d_max_key, void* d_workspace,
                          hipStream_t stream) {
  Plan plan;
  const char* why = first_refusal({
      level < 2 || level > 128 ? "the level must be in [2, 128]" : nullptr,
      n_pieces > kMaxPieces ? "more than 2^20 pieces" : nullptr,
      n_row > PLATO_AGG_PRUNE_MAX_ELEMENTS ? "the row has 2^32 elements or more" : nullptr,
      n_pieces && !h_pieces ? "null piece table" : nullptr,
  });
  if (!why) why = bad_pieces(h_pieces, n_pieces, n_row, &plan);
  if (!why && plan.n_total)
    why = first_refusal({
        !d_row || !d_codes || !d_max_key || !d_workspace ? "null row, codes, maxima or workspace pointer" : nullptr,
        !aligned(d_row, 16) ? "the row must be 16-byte aligned" : nullptr,
        !aligned(d_codes, 4) || !aligned(d_max_key, 4) ? "the codes and the maxima must be 4-byte aligned" : nullptr,
        !aligned(d_workspace, 256) ? "workspace must be 256-byte aligned" : nullptr,
    });
  if (why) return fail(PLATO_AGG_EINVAL, why);
  if (!plan.n_total) return plato_agg_internal::clear_error();

  // the maxima of empty pieces are 0 too
  hipError_t err = hipMemsetAsync(d_max_key, 0, n_pieces * 4, stream);
  if (err != hipSuccess) return fail(PLATO_AGG_EHIP, std::string("qsgd_encode maxima: ") + hipGetErrorString(err));

  // the workspace: the pieces' first tiles, the piece table
  char* ws = static_cast<char*>(d_workspace);
  uint32_t* first_tile = reinterpret_cast<uint32_t*>(ws);
  plato_agg_chunk* d_pieces = reinterpret_cast<plato_agg_chunk*>(ws + round_up(n_pieces * 4, 256));
  err = hipMemcpyAsync(d_pieces, h_pieces, n_pieces * sizeof(plato_agg_chunk), hipMemcpyHostToDevice, stream);
  if (err != hipSuccess) return fail(PLATO_AGG_EHIP, std::string("qsgd_encode tables: ") + hipGetErrorString(err));

  const Tiles tl = {d_pieces, first_tile, uint32_t(n_pieces), uint32_t(plan.n_tiles)};
  const uint32_t* row_bits = reinterpret_cast<const uint32_t*>(d_row);
  const dim3 grid(uint32_t(plan.n_tiles < kGrid ? plan.n_tiles : kGrid)), block(kThreads), one(1);
  hipLaunchKernelGGL(scan_kernel<true>, one, block, 0, stream, first_tile, uint32_t(n_pieces), d_pieces, nullptr);
  hipLaunchKernelGGL(max_kernel, grid, block, 0, stream, row_bits, tl, d_max_key);
  hipLaunchKernelGGL(encode_kernel, grid, block, 0, stream, row_bits, tl, d_max_key, float(level - 1),
                     synth_key(seed, kDrawStream), d_codes);
  err = hipGetLastError();
  if (err != hipSuccess) return fail(PLATO_AGG_EHIP, std::string("qsgd_encode: ") + hipGetErrorString(err));
  return plato_agg_internal::clear_error();
}

}  // extern "C"
