// ray_aim_host.h -- the argument rules of ol_aim_rays, decided on the host before any device
// call.  A header so that tests/hostaim can run the same rules without a device.
#pragma once
#include <cmath>

#include "../../include/optiland_hip.h"
#include "last_error.h"
#include "system_view.h"

namespace ol {

// OL_OK, or the code of the first rule the call breaks (its text in ol_last_error).  The
// current-device rule is the caller's: it needs the runtime.
inline int aim_check(const ol_system* sys, int64_t n_rays, int32_t wavelength_index,
                     int32_t first_surface, int32_t stop_surface, const ol_aim_params* p,
                     const ol_raygen_inputs* in, const void* const guess[6], void* const out[6],
                     const uint32_t* status) {
  if (!sys) return failf(OL_EINVAL, "ol_aim_rays: system is NULL");
  const SystemView v = system_view(sys);
  if (!v.consistent)
    return failf(OL_EINVAL, "ol_aim_rays: the system's tables are inconsistent after a failed "
                            "ol_system_update (destroy it and create a new one)");
  if (!p) return failf(OL_EINVAL, "ol_aim_rays: params is NULL");
  if (!in || !in->px || !in->py)
    return failf(OL_EINVAL, "ol_aim_rays: the pupil planes px, py are required");
  if (!status) return failf(OL_EINVAL, "ol_aim_rays: status is NULL");
  if (n_rays < 0) return failf(OL_EINVAL, "ol_aim_rays: negative ray count");
  if (!out) return failf(OL_EINVAL, "ol_aim_rays: out is NULL");
  for (int k = 0; k < 6; ++k)
    if (!out[k]) return failf(OL_EINVAL, "ol_aim_rays: out[%d] is NULL", k);
  if (guess) {
    for (int k = 0; k < 6; ++k)
      if (!guess[k]) return failf(OL_EINVAL, "ol_aim_rays: guess[%d] is NULL", k);
  } else if ((in->hx == nullptr) != (in->hy == nullptr) ||
             (in->vx == nullptr) != (in->vy == nullptr)) {
    return failf(OL_EINVAL, "ol_aim_rays: hx/hy (and vx/vy) must be given together");
  }
  if (wavelength_index < 0 || wavelength_index >= v.n_wl)
    return failf(OL_EINVAL, "ol_aim_rays: wavelength index %d outside [0, %d)", wavelength_index,
                 v.n_wl);
  if (first_surface < 0 || stop_surface >= v.n_surf || first_surface > stop_surface)
    return failf(OL_EINVAL, "ol_aim_rays: surface range [%d, %d] outside [0, %d)", first_surface,
                 stop_surface, v.n_surf);
  if (p->max_iter < 0 || p->max_iter > OL_AIM_MAX_ITER)
    return failf(OL_EINVAL, "ol_aim_rays: max_iter %d outside [0, %d]", p->max_iter,
                 OL_AIM_MAX_ITER);
  if (!(p->tol >= 0.0) || std::isinf(p->tol))
    return failf(OL_EINVAL, "ol_aim_rays: tol %g must be finite and not negative", p->tol);
  if (std::isnan(p->stop_radius) || std::isnan(p->jacobian))
    return failf(OL_EINVAL, "ol_aim_rays: stop_radius %g / jacobian %g is NaN", p->stop_radius,
                 p->jacobian);
  for (int32_t s = first_surface; s <= stop_surface; ++s)
    if (is_forbes_kind(v.geom[s]))
      return failf(OL_EUNSUPPORTED, "ol_aim_rays: surface %d is a Forbes surface (traced by "
                                    "ol_trace_forbes only)", s);
  // a batch-global stop rule has no per-ray form
  for (int32_t s = first_surface; s <= stop_surface; ++s)
    if (v.ref_newton[s])
      return failf(OL_EUNSUPPORTED, "ol_aim_rays: surface %d carries OL_SURF_REFERENCE_NEWTON "
                                    "(its iteration count is a property of the batch)", s);
  return OL_OK;
}

}  // namespace ol
