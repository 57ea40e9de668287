// entry_rules.h -- the argument rules the C entry points share, each stated ONCE: a small function
// of (who, ...) that returns OL_OK or the code of the broken rule, its text in ol_last_error.
// engine.py turns these texts into the reference's exceptions and the tests match on them
// (tests/golden/capi_rules.json pins every one, and the order in which each entry applies them).
// An entry point calls the rules in its own order and keeps written out what is its alone.
//
// Host-only and header-only: capi.hip references no symbol of the other units (tests/hostmath
// links it alone) and the other units know a system as its SystemView.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/optiland_hip.h"
#include "last_error.h"
#include "system_view.h"

namespace ol {

// false between the two uploads of ol_system_update and for good if the second one fails
inline int rule_consistent(const char* who, bool consistent) {
  if (consistent) return OL_OK;
  return failf(OL_EINVAL, "%s: the system's tables are inconsistent after a failed "
                          "ol_system_update (destroy it and create a new one)", who);
}

// not NULL and consistent; `v` is the system's view from here on
inline int rule_system(const char* who, const ol_system* sys, SystemView& v) {
  if (!sys) return failf(OL_EINVAL, "%s: system is NULL", who);
  v = system_view(sys);
  return rule_consistent(who, v.consistent);
}

inline int rule_dtype(const char* who, ol_dtype dt) {
  if (dt == OL_F32 || dt == OL_F64) return OL_OK;
  return failf(OL_EINVAL, "%s: bad dtype %d", who, (int)dt);
}

// (ol_trace_opd words its own)
inline int rule_fp64_only(const char* who, ol_dtype dt) {
  if (dt == OL_F32)
    return failf(OL_EUNSUPPORTED, "%s: wavefront work is fp64 only (an OPD in waves needs 1e-9 "
                                  "of the path length)", who);
  return rule_dtype(who, dt);
}

// `what`: "negative ray count" where rays are counted, "negative count" elsewhere
inline int rule_count(const char* who, int64_t n, const char* what) {
  return n < 0 ? failf(OL_EINVAL, "%s: %s", who, what) : OL_OK;
}

inline int rule_wavelength(const char* who, int32_t n_wl, int32_t wl) {
  if (wl >= 0 && wl < n_wl) return OL_OK;
  return failf(OL_EINVAL, "%s: wavelength index %d outside [0, %d)", who, wl, n_wl);
}

inline int rule_range(const char* who, const SystemView& v, int32_t first, int32_t last) {
  if (first >= 0 && last < v.n_surf && first <= last) return OL_OK;
  return failf(OL_EINVAL, "%s: surface range [%d, %d] outside [0, %d)", who, first, last,
               v.n_surf);
}

// an array of `k` planes: the array itself, then each plane
template <typename P>
inline int rule_planes(const char* who, const char* name, P const* planes, int k) {
  if (!planes) return failf(OL_EINVAL, "%s: %s is NULL", who, name);
  for (int i = 0; i < k; ++i)
    if (!planes[i]) return failf(OL_EINVAL, "%s: %s[%d] is NULL", who, name, i);
  return OL_OK;
}

inline int rule_stride(const char* who, int64_t record_stride, int64_t n_rays) {
  if (record_stride >= n_rays) return OL_OK;
  return failf(OL_EINVAL, "%s: record_stride %lld < n_rays %lld", who, (long long)record_stride,
               (long long)n_rays);
}

// rays/ray_generator.py:89-94 (same text): polarization-dependent coatings need polarized rays
inline int rule_polarisation_required(const SystemView& v, int32_t first, int32_t last) {
  for (int32_t s = first; s <= last; ++s)
    if (v.coating[s] >= OL_COAT_FRESNEL)
      return failf(OL_EINVAL, "Polarization must be set when surfaces have polarization-dependent "
                              "coatings.");
  return OL_OK;
}

inline int rule_retarder_needs_complex(const char* who, const SystemView& v, int32_t first,
                                       int32_t last) {
  for (int32_t s = first; s <= last; ++s)
    if (v.coating[s] == OL_COAT_RETARDER)
      return failf(OL_EINVAL, "%s: surface %d is a retarder (complex Jones matrix): pass an "
                              "18-plane prt with OL_TRACE_PRT_COMPLEX", who, s);
  return OL_OK;
}

// The one-launch surface kinds, each traced by an entry of its own (forbes.hip, grating.hip,
// phase.hip, grid_sag.hip: one launch between two fused runs).  The fused kernels carry no functor
// for them -- they would refract at a grating or a phase surface -- so every entry point that
// walks a surface range answers a range that holds one, before any launch.  The order of the
// table (the enumeration kSingle* of geom_kinds.h) is the order in which the kinds are looked for.
struct SingleKind {
  const char* entry;            // the one entry point that traces the kind
  bool (*is_kind)(int32_t);     // on an ol_geom_kind
  const char* row;              // "surface 3 is not a <row>": what that entry asks its row to be
  const char* found;            // "surface 3 is <found>": what a range is told it holds
  bool takes_wavelength_um;     // the entry has a wavelength_um argument
};
constexpr SingleKind kSingleKinds[kSingleKindCount] = {
    {"ol_trace_forbes", is_forbes_kind, "Forbes surface", "a Forbes surface", false},
    {"ol_trace_grating", is_grating_kind, "grating", "a diffraction grating", true},
    {"ol_trace_phase", is_phase_kind, "phase surface", "a phase surface", true},
    {"ol_trace_grid_sag", is_grid_sag_kind, "grid-sag surface", "a grid-sag surface", false},
};

// kinds outer, surfaces inner: a range that holds two kinds names the row of the kind that comes
// first in the table, not the row that comes first in the range
inline int rule_no_single_kinds(const char* who, const SystemView& v, int32_t first,
                                int32_t last) {
  for (const SingleKind& k : kSingleKinds)
    for (int32_t s = first; s <= last; ++s)
      if (k.is_kind(v.geom[s]))
        return failf(OL_EUNSUPPORTED, "%s: surface %d is %s: trace it with %s and cut the range "
                                      "there", who, s, k.found, k.entry);
  return OL_OK;
}

// the fused entry points (one launch: generate -> trace [-> reduce]) walk the whole system and do
// not serve ranges whose Newton iteration count is a property of the batch
inline int rule_no_reference_newton(const char* who, const SystemView& v) {
  if (int rc = rule_no_single_kinds(who, v, 0, v.n_surf - 1)) return rc;
  for (int32_t s = 0; s < v.n_surf; ++s)
    if (v.ref_newton[s])
      return failf(OL_EUNSUPPORTED, "%s: the system carries OL_SURF_REFERENCE_NEWTON surfaces "
                                    "(reference stop rule): generate with ol_generate_rays, count "
                                    "with ol_newton_count, trace with ol_trace_ex", who);
  return OL_OK;
}

// the library's one question to the runtime about the current device
inline bool current_device(int* device) { return hipGetDevice(device) == hipSuccess; }

// the tables live on one device and the launch goes to the current one
inline int rule_current_device(const char* who, const SystemView& v) {
  int cur = -1;
  if (current_device(&cur) && cur == v.device) return OL_OK;
  return failf(OL_EINVAL, "%s: current HIP device %d is not the system's device %d", who, cur,
               v.device);
}

}  // namespace ol
