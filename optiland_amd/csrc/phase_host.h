// phase_host.h -- the argument rules of ol_trace_phase, decided on the host before any device
// call.  A header so that tests/hostphase can run the same rules without a device.
#pragma once

#include <cmath>

#include "../../include/optiland_hip.h"
#include "entry_rules.h"

namespace ol {

// q = 1 / k0 of phase_device.h, in double: the reference's k0 is 2 pi / (wavelength * 1e-3)
inline double phase_q(double wavelength_um) {
  return wavelength_um * 1e-3 / (2.0 * 3.141592653589793238462643383279502884);
}

// OL_OK, or the code of the first rule the call breaks (its text in ol_last_error): the shared
// rules of entry_rules.h in the order grating_check uses, its own written out.  The
// current-device rule is the caller's: it needs the runtime.
inline int phase_check(const ol_system* sys, ol_dtype dt, int64_t n_rays, void* const rays[8],
                       int32_t wavelength_index, double wavelength_um, const void* record_row,
                       int64_t record_stride, int32_t surface, uint32_t flags) {
  SystemView v;
  if (int rc = rule_system("ol_trace_phase", sys, v)) return rc;
  if (int rc = rule_dtype("ol_trace_phase", dt)) return rc;
  if (int rc = rule_count("ol_trace_phase", n_rays, "negative ray count")) return rc;
  if (surface < 0 || surface >= v.n_surf)
    return failf(OL_EINVAL, "ol_trace_phase: surface %d outside [0, %d)", surface, v.n_surf);
  if (!is_phase_kind(v.geom[surface]))
    return failf(OL_EINVAL, "ol_trace_phase: surface %d is not a phase surface (geometry kind "
                            "%d): trace it with ol_trace", surface, v.geom[surface]);
  if (int rc = rule_wavelength("ol_trace_phase", v.n_wl, wavelength_index)) return rc;
  if (!(std::isfinite(wavelength_um) && wavelength_um > 0.0))
    return failf(OL_EINVAL, "ol_trace_phase: wavelength_um %g must be finite and greater "
                            "than 0", wavelength_um);
  if (flags & ~(uint32_t)(OL_TRACE_WRITE_RAYS | OL_TRACE_MIDRANGE))
    return failf(OL_EINVAL, "ol_trace_phase: flags 0x%x: OL_TRACE_WRITE_RAYS and "
                            "OL_TRACE_MIDRANGE only", flags);
  if (v.coating[surface] >= OL_COAT_FRESNEL)
    return failf(OL_EUNSUPPORTED, "ol_trace_phase: surface %d carries a polarisation-dependent "
                                  "coating (unpolarised launches only)", surface);
  if (n_rays == 0) return OL_OK;   // nothing is read or written
  if (n_rays > (int64_t)0x7fffffff * 64)
    return failf(OL_EINVAL, "ol_trace_phase: %lld rays are more than one launch takes",
                 (long long)n_rays);
  if (int rc = rule_planes("ol_trace_phase", "rays", rays, 8)) return rc;
  if (record_row)
    if (int rc = rule_stride("ol_trace_phase", record_stride, n_rays)) return rc;
  if (!record_row && !(flags & OL_TRACE_WRITE_RAYS))
    return failf(OL_EINVAL, "ol_trace_phase: nothing to write (no record_row, no "
                            "OL_TRACE_WRITE_RAYS)");
  return OL_OK;
}

}  // namespace ol
