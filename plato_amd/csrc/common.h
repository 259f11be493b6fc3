// Internal helpers shared by the HIP translation units of libplato_agg.so
// (not part of the C ABI).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cmath>
#include <mutex>
#include <string>

namespace plato_agg_internal {

// Sets the thread-local message returned by plato_agg_last_error() and
// returns `code` (a PLATO_AGG_E* status).
__attribute__((visibility("hidden"))) int set_error(int code, const std::string& msg);

// Clears the message; returns PLATO_AGG_OK.
__attribute__((visibility("hidden"))) int clear_error();

// The kernels that replace a float32 division p / d by float(double(p) * (1.0 / double(d))) (qsgd.hip
// decode_tab / decode_arith, fedadp.hip adp_div_lr_f64) get the IEEE quotient's bits for every float p
// iff this holds for d: d is not an even integer, or |d| is a power of two (exact reciprocal).
// A quotient of two floats is either exactly on a midpoint of the float grid or at least ~2^-49
// (relative) away from one, and the float64 product is within 2^-52 of the quotient, so only an exact
// midpoint can round differently.  A midpoint between normal floats needs 25 significant bits and is
// never a quotient of two floats unless d is a power of two.  A midpoint between two float32
// subnormals, an odd multiple of 2^-150, is one when p = odd * (d / 2) * 2^-149 is a float: d an even
// integer.  There the inexact reciprocal puts the product beside the tie, which then rounds to the
// nearer subnormal where IEEE division rounds to even (d = 98, p = 147 * 2^-149: 2^-149 against
// 2^-148; tests/test_division.py).  Zero, infinite and NaN divisors are safe (both forms give the same
// zeros, infinities and NaNs).  Callers route an unsafe divisor to the IEEE division.
inline bool recip_product_exact(float d) {
  const float a = std::fabs(d);
  if (!(a >= 2.f) || std::isinf(a)) return true;  // no even integer below 2
  int e;
  if (std::frexp(a, &e) == 0.5f) return true;  // a power of two
  return std::fmod(a, 2.f) != 0.f;
}

// A second stream per device (created on first use, never destroyed) with a fork / join event pair, so
// that independent launches of one C-ABI call overlap: record `fork` on the caller's stream and make `s`
// wait for it, launch on `s`, then record `join` on `s` and make the caller's stream wait for it.  The
// sequence runs under `mu` (the events are reused across calls; a wait captures an event's state when it
// is enqueued), so concurrent callers stay ordered.  Defined in flat.hip.
struct SideStream {
  hipStream_t s = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
  std::mutex mu;
};
__attribute__((visibility("hidden"))) SideStream* side_stream(int dev);

}  // namespace plato_agg_internal
