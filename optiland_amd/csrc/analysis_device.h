// analysis_device.h -- device helpers the fp64 analysis kernels share (huygens.hip, mtf.hip,
// zernike_fit.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <limits>

namespace ol {

// neither NaN nor +-inf
__device__ __forceinline__ bool is_finite(double v) {
  return fabs(v) <= std::numeric_limits<double>::max();
}

// The argument x of sincospi(2 x) for a phase of t (+ t_lo) cycles: t - rint(t) is exact, so
// sincospi sees |argument| <= 1.  (Two overloads: t_lo = 0 would turn a -0.0 into +0.0, and the
// sign of a zero sine with it.)
__device__ __forceinline__ double phase_cycles(double t) { return t - rint(t); }
__device__ __forceinline__ double phase_cycles(double t, double t_lo) {
  return (t - rint(t)) + t_lo;
}

}  // namespace ol
