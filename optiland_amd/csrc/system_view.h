// system_view.h -- what a translation unit other than capi.hip may know of an `ol_system`: the
// fp64 device table and the host-side facts the entry points validate against.  `ol_system`
// itself stays private to capi.hip, which defines the two functions below; capi.hip references
// no symbol of the units that use them (tests/hostmath links it alone).  The rules every entry
// point checks a system and its arguments against are functions of this view: entry_rules.h.
#pragma once
#include <stdint.h>

#include "../../include/optiland_hip.h"
#include "device_table.h"
#include "geom_kinds.h"

namespace ol {

struct SystemView {
  int32_t n_surf, n_wl;
  int device;
  bool consistent;   // false after a failed ol_system_update: every entry point refuses it
  const DevSurfHot<double>* surf;
  const DevSurfCold<double>* cold;
  const DevOptics<double>* optics;   // [n_surf][n_wl]
  const double* coeffs;
  const int32_t* interaction;        // host copies, [n_surf]
  const int32_t* coating;
  const uint8_t* ref_newton;         // OL_SURF_REFERENCE_NEWTON on a traced Newton surface
  const int32_t* geom;               // ol_geom_kind as given, [n_surf]
  const DevSurfHot<float>* surf32;   // the fp32 table (single_surface.h: rows_of<float>)
  const DevSurfCold<float>* cold32;
  const DevOptics<float>* optics32;
  const float* coeffs32;
};

// on an ol_geom_kind: the one-launch column of geom_kinds.h
inline bool is_forbes_kind(int32_t g) { return single_kind(g) == kSingleForbes; }
inline bool is_grating_kind(int32_t g) { return single_kind(g) == kSingleGrating; }
inline bool is_phase_kind(int32_t g) { return single_kind(g) == kSinglePhase; }
inline bool is_grid_sag_kind(int32_t g) { return single_kind(g) == kSingleGridSag; }

// `sys` must not be NULL
SystemView system_view(const ol_system* sys);
// the Newton kernel family of [first, last] (device_table.h kNr*), as ol_trace chooses it
int system_newton_family(const ol_system* sys, int32_t first, int32_t last);

}  // namespace ol
