// forbes_host.h -- the argument rules of ol_trace_forbes, decided on the host before any device
// call: single_check (single_host.h) for this kind.  A header so that tests/hostforbes can run the
// same rules without a device.
#pragma once
#include "single_host.h"

namespace ol {

inline int forbes_check(const ol_system* sys, ol_dtype dt, int64_t n_rays, void* const rays[8],
                        int32_t wavelength_index, const void* record_row,
                        int64_t record_stride, int32_t surface, uint32_t flags) {
  return single_check(kSingleKinds[kSingleForbes], sys, dt, n_rays, rays, wavelength_index,
                      nullptr, record_row, record_stride, surface, flags);
}

}  // namespace ol
