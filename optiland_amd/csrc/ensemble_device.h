// ensemble_device.h -- the variant lookup of an ensemble launch (ol_trace_spot_ensemble): from a
// cell of the launch grid to the table rows, the ray-generation constants and the field point that
// cell traces with.
//
// An ol_ensemble holds K variants of ONE optic -- same structure, other values -- as four STACKED
// tables per precision plus one RaygenConsts<T> per variant:
//   surf   [K][n_surf]         hot rows            cold   [K][n_surf]   cold rows
//   optics [K][n_surf][n_wl]   index rows          coeffs [K][coef_cap] coefficient blocks
// Variant v's tables are `base + v * stride`: the same rows an ol_system of that variant alone
// would hold (coeff_off counts inside the variant's own coefficient block), so the surface walk of
// the fused spot kernel runs on them unchanged.  The ray-generation constants are per variant
// because they are not structure: a radius in front of the stop moves the entrance pupil (EPL,
// EPD), a first thickness moves the launch plane.
//
// Everything here depends on the CELL only -- the workgroup's place in the launch grid -- so in
// device code every load is a scalar load (constant address space) and every result lives in
// SGPRs; nothing per lane knows which variant it traces.  Compiles for the host too (OL_HOST_MATH:
// tests/hostensemble walks the same cells on the CPU).
#pragma once
#include <stdint.h>

#include "../../include/optiland_hip.h"
#include "device_table.h"
#include "raygen_device.h"

namespace ol {

constexpr uint32_t kStatusEnsembleCell = 0x40u;  // OL_STATUS_ENSEMBLE_CELL

template <typename T>
struct EnsembleTables {
  const DevSurfHot<T>* surf;
  const DevSurfCold<T>* cold;
  const DevOptics<T>* optics;
  const T* coeffs;
  const RaygenConsts<T>* rgc;   // [K]
  int32_t n_variants, n_surf, n_wl;
  int32_t coef_cap;             // elements between two variants' coefficient blocks
};

// linear cell index of a workgroup: the cells fill blockIdx.y first, then blockIdx.z (a grid
// dimension ends at 65535, a tolerancing run does not)
OL_DEV int64_t ensemble_cell_index(uint32_t by, uint32_t bz, uint32_t grid_y) {
  return (int64_t)bz * grid_y + by;
}

// the (y, z) extent of a launch grid that holds `n_cells` cells: z as small as it can be, y the
// even share -- at most z - 1 workgroup rows past the end, each of which leaves at once
inline void ensemble_grid(int64_t n_cells, uint32_t& grid_y, uint32_t& grid_z) {
  constexpr int64_t kMaxDim = 65535;
  const int64_t z = (n_cells + kMaxDim - 1) / kMaxDim;
  grid_z = (uint32_t)(z > 0 ? z : 1);
  grid_y = (uint32_t)((n_cells + grid_z - 1) / grid_z);
}
constexpr int64_t kEnsembleMaxCells = (int64_t)65535 * 65535;

// a cell may only name what the ensemble holds: checked BEFORE any table address is formed (the
// cells are device memory the host never sees)
template <typename T>
OL_DEV bool ensemble_cell_ok(const EnsembleTables<T>& t, int32_t variant, int32_t wl) {
  return variant >= 0 && variant < t.n_variants && wl >= 0 && wl < t.n_wl;
}

// the rows one cell traces with: variant `v`'s tables, the optics rows offset to wavelength `wl`
// (row of surface s: optics + s * n_wl)
template <typename T>
struct EnsembleRows {
  cptr<DevSurfHot<T>> surf;
  cptr<DevSurfCold<T>> cold;
  cptr<DevOptics<T>> optics;
  cptr<T> coeffs;
  cptr<RaygenConsts<T>> rgc;
};

template <typename T>
OL_DEV EnsembleRows<T> ensemble_rows(const EnsembleTables<T>& t, int32_t v, int32_t wl) {
  const int64_t row0 = (int64_t)v * t.n_surf;
  EnsembleRows<T> r;
  r.surf = as_const(t.surf) + row0;
  r.cold = as_const(t.cold) + row0;
  r.optics = as_const(t.optics) + (row0 * t.n_wl + wl);
  r.coeffs = as_const(t.coeffs) + (int64_t)v * t.coef_cap;
  r.rgc = as_const(t.rgc) + v;
  return r;
}

// the field point of a cell in the working precision: the tangents (or object heights) exactly as
// a per-ray field plane would give them (raygen_field on the VARIANT's constants), the
// vignetting factors, the centre of the moments
template <typename T>
struct EnsembleField {
  T tx, ty, vx, vy;
  double cx, cy;
};

template <typename T>
OL_DEV EnsembleField<T> ensemble_field(const RaygenConsts<T>& c, cptr<ol_ensemble_cell> cell,
                                       uint32_t rg_flags, uint32_t& status) {
  EnsembleField<T> f;
  const T hx = (T)cell->hx, hy = (T)cell->hy;
  if ((rg_flags & kRaygenCheckField) && (outside_unit(hx) || outside_unit(hy)))
    status |= kStatusFieldRange;
  raygen_field<T>(c, hx, hy, f.tx, f.ty);
  f.vx = (T)cell->vx;
  f.vy = (T)cell->vy;
  f.cx = cell->cx;
  f.cy = cell->cy;
  return f;
}

// The surface walk of one lane's rays through the cell's variant, and the way back to the global
// frame: spot_trace_kernel's loop (trace_kernel.hip) on the rows of `ensemble_rows`.  FETCH: the
// rows are re-read phase by phase (SurfFetched: the Newton and fp64 kernels, which are short of
// scalar registers); otherwise the hot block and the optics row are loaded once per surface, the
// hot block one surface ahead.  `r`: the rays in the global frame on entry; `g`: the final state
// in the global frame, or (keep_local) in the last traced surface's own.
template <typename T, typename V, int NV, int NR, bool PAIR, bool FETCH>
OL_DEV void ensemble_walk(const EnsembleRows<T>& rows, int n_surf, int n_wl, bool keep_local,
                          Ray<V> (&r)[NV], Ray<V> (&g)[NV], uint32_t& status) {
  bool is_global = true, prt_fresh = false;  // (unpolarised: no PRT matrix is carried)
  Prt<T, 0> P[1];
  if constexpr (FETCH) {
    int last_idx = 0;
    for (int s = 0; s < n_surf; ++s) {
      const SurfFetched<T> h{rows.surf + s, rows.cold + s, rows.optics + s * n_wl};
      if (refresh(h.hot)->interaction != kRecordOnly) {
        surface_step<V, NV, 0, NR, PAIR>(h, rows.coeffs, is_global, r, P, status, prt_fresh);
        is_global = false;
        last_idx = s;
      }
    }
    const DevSurf<T> lt =
        SurfFetched<T>{rows.surf + last_idx, rows.cold + last_idx, rows.optics}.surf();
    const bool keep = is_global || keep_local;
    for (int j = 0; j < NV; ++j) g[j] = keep ? r[j] : to_global<V>(lt, r[j]);
  } else {
    DevSurf<T> last_traced;
    static_cast<DevSurfHot<T>&>(last_traced) = load_hot<T>(rows.surf);
    last_traced.cold = rows.cold;
    DevSurfHot<T> cur = load_hot<T>(rows.surf);
    for (int s = 0; s < n_surf; ++s) {
      DevSurf<T> S;
      static_cast<DevSurfHot<T>&>(S) = cur;
      if (s + 1 < n_surf) cur = load_hot<T>(rows.surf + (s + 1));
      S.cold = rows.cold + s;
      if (S.interaction != kRecordOnly) {
        const DevOptics<T> O = load_optics<T>(rows.optics + s * n_wl);
        surface_step<V, NV, 0, NR, PAIR>(S, O, rows.coeffs, is_global, r, P, status, prt_fresh);
        is_global = false;
        last_traced = S;
      }
    }
    const bool keep = is_global || keep_local;
    for (int j = 0; j < NV; ++j) g[j] = keep ? r[j] : to_global<V>(last_traced, r[j]);
  }
}

}  // namespace ol
