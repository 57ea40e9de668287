// geom_kinds.h -- what the host side knows of each public geometry kind (ol_geom_kind in
// include/optiland_hip.h), one row per kind: staging (system_stage.h), the kind predicates
// (system_view.h) and through them the entry rules (entry_rules.h) all read this table.  Data only
// -- the device translation units see it through system_view.h.  A new kind adds its row here and
// its block stager in system_stage.h.
#pragma once
#include <stdint.h>

#include "../../include/optiland_hip.h"
#include "device_table.h"

namespace ol {

// the one-launch kinds, in the order entry_rules.h: kSingleKinds looks for them
enum { kSingleForbes, kSingleGrating, kSinglePhase, kSingleGridSag, kSingleKindCount };
constexpr int kSingleNone = -1;

struct GeomKind {
  int kind;             // its own ol_geom_kind; -1: the number names no kind
  int device;           // kGeom* of device_table.h (a Zernike row may still become kGeomZernikeMono)
  int per, extra;       // doubles per n_coeff unit of the public block, and doubles in front of them
  bool flat;            // no base conic: kSurfRadiusInf whatever the row's radius says
  bool reference_root;  // OL_SURF_REFERENCE_ROOT applies
  bool newton;          // OL_SURF_REFERENCE_NEWTON applies (a traced Newton-Raphson surface)
  int single;           // kSingle* of the entry that traces it, or kSingleNone
};

constexpr GeomKind kNoGeomKind = {-1, -1, 0, 0, false, false, false, kSingleNone};
constexpr GeomKind kGeomKinds[] = {
    {OL_GEOM_PLANE, kGeomPlane, 1, 0, true, false, false, kSingleNone},
    {OL_GEOM_STANDARD, kGeomStandard, 1, 0, false, true, false, kSingleNone},
    {OL_GEOM_EVEN_ASPHERE, kGeomEvenAsphere, 1, 0, false, false, true, kSingleNone},
    {OL_GEOM_ZERNIKE, kGeomZernike, 4, 0, false, false, true, kSingleNone},
    {OL_GEOM_ODD_ASPHERE, kGeomOddAsphere, 1, 0, false, false, true, kSingleNone},
    {OL_GEOM_POLYNOMIAL, kGeomPolynomial, 1, 0, false, false, true, kSingleNone},
    {OL_GEOM_CHEBYSHEV, kGeomChebyshev, 1, 2, false, false, true, kSingleNone},
    {OL_GEOM_BICONIC, kGeomBiconic, 1, 0, false, false, true, kSingleNone},
    {OL_GEOM_TOROIDAL, kGeomToroidal, 1, 0, false, false, true, kSingleNone},
    {OL_GEOM_FORBES_Q, kGeomForbesQ, 1, 0, false, false, true, kSingleForbes},
    {OL_GEOM_FORBES_Q2D, kGeomForbesQ2d, 1, 0, false, false, true, kSingleForbes},
    {OL_GEOM_PLANE_GRATING, kGeomPlaneGrating, 1, 0, true, false, false, kSingleGrating},
    {OL_GEOM_STANDARD_GRATING, kGeomStandardGrating, 1, 0, false, true, false, kSingleGrating},
    kNoGeomKind,   // 13: never assigned
    {OL_GEOM_PLANE_PHASE, kGeomPlanePhase, 1, 0, true, false, false, kSinglePhase},
    kNoGeomKind,   // 15: never assigned
    {OL_GEOM_GRID_SAG, kGeomGridSag, 1, 0, true, false, false, kSingleGridSag},
};
constexpr int kGeomKindCount = sizeof(kGeomKinds) / sizeof(kGeomKinds[0]);

constexpr bool geom_kinds_in_order() {
  for (int g = 0; g < kGeomKindCount; ++g)
    if (kGeomKinds[g].kind != g && kGeomKinds[g].kind != -1) return false;
  return true;
}
static_assert(geom_kinds_in_order(), "row g of kGeomKinds describes ol_geom_kind g");

// the row of an ol_geom_kind, NULL for a number that names no kind
constexpr const GeomKind* geom_kind(int32_t g) {
  return g >= 0 && g < kGeomKindCount && kGeomKinds[g].kind == g ? &kGeomKinds[g] : nullptr;
}

// kSingle* of an ol_geom_kind, kSingleNone for every other number
constexpr int single_kind(int32_t g) {
  return geom_kind(g) ? geom_kind(g)->single : kSingleNone;
}

}  // namespace ol
