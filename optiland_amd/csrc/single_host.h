// single_host.h -- the argument rules of the four one-surface entries (ol_trace_forbes,
// ol_trace_grating, ol_trace_phase, ol_trace_grid_sag), decided on the host before any device
// call.  A header so that tests/hostforbes, hostgrating, hostphase and hostgrid can run the same
// rules without a device.
#pragma once

#include <cmath>

#include "../../include/optiland_hip.h"
#include "entry_rules.h"

namespace ol {

// OL_OK, or the code of the first rule the call breaks (its text in ol_last_error): the shared
// rules of entry_rules.h in these entries' order, their own written out.  `kind`: the entry's row
// of kSingleKinds; `wavelength_um`: NULL for an entry that takes none.  The current-device rule
// is the caller's: it needs the runtime.
inline int single_check(const SingleKind& kind, const ol_system* sys, ol_dtype dt, int64_t n_rays,
                        void* const rays[8], int32_t wavelength_index,
                        const double* wavelength_um, const void* record_row,
                        int64_t record_stride, int32_t surface, uint32_t flags) {
  const char* who = kind.entry;
  SystemView v;
  if (int rc = rule_system(who, sys, v)) return rc;
  if (int rc = rule_dtype(who, dt)) return rc;
  if (int rc = rule_count(who, n_rays, "negative ray count")) return rc;
  if (surface < 0 || surface >= v.n_surf)
    return failf(OL_EINVAL, "%s: surface %d outside [0, %d)", who, surface, v.n_surf);
  if (!kind.is_kind(v.geom[surface]))
    return failf(OL_EINVAL, "%s: surface %d is not a %s (geometry kind %d): trace it with "
                            "ol_trace", who, surface, kind.row, v.geom[surface]);
  if (int rc = rule_wavelength(who, v.n_wl, wavelength_index)) return rc;
  if (kind.takes_wavelength_um && !(std::isfinite(*wavelength_um) && *wavelength_um > 0.0))
    return failf(OL_EINVAL, "%s: wavelength_um %g must be finite and greater than 0", who,
                 *wavelength_um);
  if (flags & ~(uint32_t)(OL_TRACE_WRITE_RAYS | OL_TRACE_MIDRANGE))
    return failf(OL_EINVAL, "%s: flags 0x%x: OL_TRACE_WRITE_RAYS and OL_TRACE_MIDRANGE only", who,
                 flags);
  if (v.coating[surface] >= OL_COAT_FRESNEL)
    return failf(OL_EUNSUPPORTED, "%s: surface %d carries a polarisation-dependent coating "
                                  "(unpolarised launches only)", who, surface);
  if (n_rays == 0) return OL_OK;   // nothing is read or written
  if (n_rays > (int64_t)0x7fffffff * 64)
    return failf(OL_EINVAL, "%s: %lld rays are more than one launch takes", who,
                 (long long)n_rays);
  if (int rc = rule_planes(who, "rays", rays, 8)) return rc;
  if (record_row)
    if (int rc = rule_stride(who, record_stride, n_rays)) return rc;
  if (!record_row && !(flags & OL_TRACE_WRITE_RAYS))
    return failf(OL_EINVAL, "%s: nothing to write (no record_row, no OL_TRACE_WRITE_RAYS)", who);
  return OL_OK;
}

}  // namespace ol
