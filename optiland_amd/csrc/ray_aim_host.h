// ray_aim_host.h -- the argument rules of ol_aim_rays, decided on the host before any device
// call.  A header so that tests/hostaim can run the same rules without a device.
#pragma once
#include <cmath>

#include "../../include/optiland_hip.h"
#include "entry_rules.h"

namespace ol {

// OL_OK, or the code of the first rule the call breaks (its text in ol_last_error): the shared
// rules of entry_rules.h in this entry's order, its own written out.  The current-device rule is
// the caller's: it needs the runtime.
inline int aim_check(const ol_system* sys, int64_t n_rays, int32_t wavelength_index,
                     int32_t first_surface, int32_t stop_surface, const ol_aim_params* p,
                     const ol_raygen_inputs* in, const void* const guess[6], void* const out[6],
                     const uint32_t* status) {
  SystemView v;
  if (int rc = rule_system("ol_aim_rays", sys, v)) return rc;
  if (!p) return failf(OL_EINVAL, "ol_aim_rays: params is NULL");
  if (!in || !in->px || !in->py)
    return failf(OL_EINVAL, "ol_aim_rays: the pupil planes px, py are required");
  if (!status) return failf(OL_EINVAL, "ol_aim_rays: status is NULL");
  if (int rc = rule_count("ol_aim_rays", n_rays, "negative ray count")) return rc;
  if (int rc = rule_planes("ol_aim_rays", "out", out, 6)) return rc;
  if (guess) {
    if (int rc = rule_planes("ol_aim_rays", "guess", guess, 6)) return rc;
  } else if ((in->hx == nullptr) != (in->hy == nullptr) ||
             (in->vx == nullptr) != (in->vy == nullptr)) {
    return failf(OL_EINVAL, "ol_aim_rays: hx/hy (and vx/vy) must be given together");
  }
  if (int rc = rule_wavelength("ol_aim_rays", v.n_wl, wavelength_index)) return rc;
  if (int rc = rule_range("ol_aim_rays", v, first_surface, stop_surface)) return rc;
  if (p->max_iter < 0 || p->max_iter > OL_AIM_MAX_ITER)
    return failf(OL_EINVAL, "ol_aim_rays: max_iter %d outside [0, %d]", p->max_iter,
                 OL_AIM_MAX_ITER);
  if (!(p->tol >= 0.0) || std::isinf(p->tol))
    return failf(OL_EINVAL, "ol_aim_rays: tol %g must be finite and not negative", p->tol);
  if (std::isnan(p->stop_radius) || std::isnan(p->jacobian))
    return failf(OL_EINVAL, "ol_aim_rays: stop_radius %g / jacobian %g is NaN", p->stop_radius,
                 p->jacobian);
  // (this entry words the two range rules its own way; the kinds in the order of
  // rule_no_single_kinds)
  for (const SingleKind& k : kSingleKinds)
    for (int32_t s = first_surface; s <= stop_surface; ++s)
      if (k.is_kind(v.geom[s]))
        return failf(OL_EUNSUPPORTED, "ol_aim_rays: surface %d is %s (traced by %s only)", s,
                     k.found, k.entry);
  // a batch-global stop rule has no per-ray form
  for (int32_t s = first_surface; s <= stop_surface; ++s)
    if (v.ref_newton[s])
      return failf(OL_EUNSUPPORTED, "ol_aim_rays: surface %d carries OL_SURF_REFERENCE_NEWTON "
                                    "(its iteration count is a property of the batch)", s);
  return OL_OK;
}

}  // namespace ol
