// phase_host.h -- the argument rules of ol_trace_phase, decided on the host before any device
// call: single_check (single_host.h) for this kind.  A header so that tests/hostphase can run the
// same rules without a device.
#pragma once
#include "single_host.h"

namespace ol {

// q = 1 / k0 of phase_device.h, in double: the reference's k0 is 2 pi / (wavelength * 1e-3)
inline double phase_q(double wavelength_um) {
  return wavelength_um * 1e-3 / (2.0 * 3.141592653589793238462643383279502884);
}

inline int phase_check(const ol_system* sys, ol_dtype dt, int64_t n_rays, void* const rays[8],
                       int32_t wavelength_index, double wavelength_um, const void* record_row,
                       int64_t record_stride, int32_t surface, uint32_t flags) {
  return single_check(kSingleKinds[kSinglePhase], sys, dt, n_rays, rays, wavelength_index,
                      &wavelength_um, record_row, record_stride, surface, flags);
}

}  // namespace ol
