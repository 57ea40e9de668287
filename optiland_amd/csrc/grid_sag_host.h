// grid_sag_host.h -- the argument rules of ol_trace_grid_sag, decided on the host before any
// device call.  A header so that tests/hostgrid can run the same rules without a device.
#pragma once

#include "../../include/optiland_hip.h"
#include "entry_rules.h"

namespace ol {

// OL_OK, or the code of the first rule the call breaks (its text in ol_last_error): the shared
// rules of entry_rules.h in the order forbes_check uses, its own written out.  The current-device
// rule is the caller's: it needs the runtime.
inline int grid_sag_check(const ol_system* sys, ol_dtype dt, int64_t n_rays, void* const rays[8],
                          int32_t wavelength_index, const void* record_row,
                          int64_t record_stride, int32_t surface, uint32_t flags) {
  SystemView v;
  if (int rc = rule_system("ol_trace_grid_sag", sys, v)) return rc;
  if (int rc = rule_dtype("ol_trace_grid_sag", dt)) return rc;
  if (int rc = rule_count("ol_trace_grid_sag", n_rays, "negative ray count")) return rc;
  if (surface < 0 || surface >= v.n_surf)
    return failf(OL_EINVAL, "ol_trace_grid_sag: surface %d outside [0, %d)", surface, v.n_surf);
  if (!is_grid_sag_kind(v.geom[surface]))
    return failf(OL_EINVAL, "ol_trace_grid_sag: surface %d is not a grid-sag surface (geometry "
                            "kind %d): trace it with ol_trace", surface, v.geom[surface]);
  if (int rc = rule_wavelength("ol_trace_grid_sag", v.n_wl, wavelength_index)) return rc;
  if (flags & ~(uint32_t)(OL_TRACE_WRITE_RAYS | OL_TRACE_MIDRANGE))
    return failf(OL_EINVAL, "ol_trace_grid_sag: flags 0x%x: OL_TRACE_WRITE_RAYS and "
                            "OL_TRACE_MIDRANGE only", flags);
  if (v.coating[surface] >= OL_COAT_FRESNEL)
    return failf(OL_EUNSUPPORTED, "ol_trace_grid_sag: surface %d carries a polarisation-dependent "
                                  "coating (unpolarised launches only)", surface);
  if (n_rays == 0) return OL_OK;   // nothing is read or written
  if (n_rays > (int64_t)0x7fffffff * 64)
    return failf(OL_EINVAL, "ol_trace_grid_sag: %lld rays are more than one launch takes",
                 (long long)n_rays);
  if (int rc = rule_planes("ol_trace_grid_sag", "rays", rays, 8)) return rc;
  if (record_row)
    if (int rc = rule_stride("ol_trace_grid_sag", record_stride, n_rays)) return rc;
  if (!record_row && !(flags & OL_TRACE_WRITE_RAYS))
    return failf(OL_EINVAL, "ol_trace_grid_sag: nothing to write (no record_row, no "
                            "OL_TRACE_WRITE_RAYS)");
  return OL_OK;
}

}  // namespace ol
