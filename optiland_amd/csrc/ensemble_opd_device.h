// ensemble_opd_device.h -- one cell of an ensemble WAVEFRONT launch (ol_trace_opd_ensemble): from
// the cell record to the reference sphere / plane of its chief ray and to the OPD of one pupil
// point, on the rows `ensemble_rows` selects.
//
// The pieces are the single launches': the chief ray and what it is turned into are
// chief_ref_kernel's (trace_kernel.hip), a ray's OPD is opd_trace_kernel's -- generate
// (raygen_device.h), walk (ensemble_walk), final_propagate + wavefront_one (wavefront_device.h).
// What the single launches take from the HOST and a cell cannot (it is device memory, and the
// constants are its VARIANT's) is formed here: the field tangents (raygen_field), the launch-plane
// tilt from them, half the variant's entrance-pupil diameter, the reciprocal wavelength.
//
// Everything depends on the cell only, so in device code every load is a scalar load and no lane
// knows its variant.  fp64 only, like every wavefront kernel.  Compiles for the host too
// (OL_HOST_MATH: tests/hostensemble_opd walks the same cells on the CPU).
#pragma once
#include <stdint.h>

#include "../../include/optiland_hip.h"
#include "ensemble_device.h"
#include "wavefront_device.h"

namespace ol {

// the field point of a cell: tangents (or object heights) from the VARIANT's constants, the
// vignetting factors
struct OpdCellField {
  double tx, ty, vx, vy;
};

OL_DEV OpdCellField opd_cell_field(const RaygenConsts<double>& c, cptr<ol_ensemble_opd_cell> cell,
                                   uint32_t rg_flags, uint32_t& status) {
  OpdCellField f;
  const double hx = cell->hx, hy = cell->hy;
  if ((rg_flags & kRaygenCheckField) && (outside_unit(hx) || outside_unit(hy)))
    status |= kStatusFieldRange;
  raygen_field<double>(c, hx, hy, f.tx, f.ty);
  f.vx = cell->vx;
  f.vy = cell->vy;
  return f;
}

// What ol_wavefront_reference is handed in its ol_wavefront_params, for one cell: n_image,
// 1 / wavelength, the last thickness and the reference kind from the record; half the VARIANT's
// entrance-pupil diameter; the direction cosines of the launch-plane tilt -- zero unless the
// object is at infinity and the field is an angle (wavefront/strategy.py:113-117), else
// (tx, ty, 1) / |(tx, ty, 1)| of the field tangents (:119-130).  Centre, radius, normal and
// opd_ref are the chief ray's to fill in.
OL_DEV WavefrontConsts<double> opd_cell_consts(const RaygenConsts<double>& c,
                                               cptr<ol_ensemble_opd_cell> cell, double tx,
                                               double ty) {
  WavefrontConsts<double> w;
  w.xc = w.yc = w.zc = w.R = 0.0;
  w.ni = cell->n_image;
  w.inv_w = 1.0 / (cell->wavelength_um * 1e-3);
  w.ux = w.uy = 0.0;
  if (c.infinite && !c.linear) {
    const double uz = 1.0 / sqrt(1.0 + tx * tx + ty * ty);
    w.ux = tx * uz;
    w.uy = ty * uz;
  }
  w.half_epd = c.EPD / 2.0;
  w.opd_ref = 0.0;
  w.nx = w.ny = w.nz = 0.0;
  w.last_t = cell->last_thickness;
  w.last_absorb = 0.0;   // (attenuates the chief ray ol_wavefront_reference hands back: not kept)
  w.planar = cell->planar != 0;
  return w;
}

// One ray of a cell from its pupil point to the global frame behind the last surface:
// generate on the variant's constants (read where they are used: they die with the generator),
// then the walk.  (px, py) as the CALLER passed them; a prescaled pupil is the generator's alone.
template <int NR, bool APOD, bool FETCH>
OL_DEV Ray<double> opd_cell_ray(const EnsembleRows<double>& rows, int n_surf, int n_wl,
                                const OpdCellField& f, uint32_t rg_flags, double px, double py,
                                uint32_t& status) {
  Ray<double> r[1], g[1];
  {
    const RaygenConsts<double> c = load_consts(refresh(rows.rgc));
    double vx = f.vx, vy = f.vy, o[6];
    raygen_pupil<double>(rg_flags, vx, vy, px, py, status);
    raygen_one<double>(c, f.tx, f.ty, px, py, vx, vy, o);
    r[0].x = o[0]; r[0].y = o[1]; r[0].z = o[2];
    r[0].L = o[3]; r[0].M = o[4]; r[0].N = o[5];
    if constexpr (APOD) r[0].i = raygen_apodize<double>(c, px, py); else r[0].i = 1.0;
    r[0].opd = 0.0;
  }
  ensemble_walk<double, double, 1, NR, false, FETCH>(rows, n_surf, n_wl, false, r, g, status);
  return g[0];
}

// The chief ray of a cell turned into its reference: chief_ref_kernel's tail.  Centre = the chief
// ray's image point; R = its distance to (0, 0, pupil_z) (strategy.py:228-243), or the plane
// through it normal to the chief ray (:260-284); opd_ref = the chief ray's own path to that
// surface (its pupil point is (0, 0): no tilt term).
OL_DEV void opd_cell_reference(WavefrontConsts<double>& w, Ray<double> g, double pupil_z) {
  using m = Math<double>;
  final_propagate<double, true>(w, g);
  w.xc = g.x; w.yc = g.y; w.zc = g.z;
  double t_back;
  if (w.planar) {
    w.R = 0.0;
    w.nx = g.L; w.ny = g.M; w.nz = g.N;
    t_back = 0.0;  // the chief ray's image point lies ON the plane
  } else {
    const double dz = g.z - pupil_z;
    w.R = m::sqrt(g.x * g.x + g.y * g.y + dz * dz);
    w.nx = w.ny = w.nz = 0.0;
    // path_length of the chief ray itself: the sphere is centred on its image point
    const double aa = g.L * g.L + g.M * g.M + g.N * g.N;
    const double d = 4.0 * aa * w.R * w.R;
    const double sq = m::sqrt(d < 0.0 ? 0.0 : d);
    const double t1 = m::div(-sq, 2.0 * aa), t2 = m::div(sq, 2.0 * aa);
    t_back = t1 < 0.0 ? t2 : t1;
  }
  w.opd_ref = g.opd - w.ni * t_back;
}

// ensemble_chief_kernel's body for one cell (the caller has checked the cell): the reference of
// the cell's chief ray, NR the Newton family of the walk (0, or the generic one: cold)
template <int NR>
OL_DEV WavefrontConsts<double> opd_cell_chief(const EnsembleRows<double>& rows, int n_surf,
                                              int n_wl, cptr<ol_ensemble_opd_cell> cell,
                                              uint32_t rg_flags, uint32_t& status) {
  const RaygenConsts<double> c = load_consts(rows.rgc);
  const OpdCellField f = opd_cell_field(c, cell, rg_flags, status);
  WavefrontConsts<double> w = opd_cell_consts(c, cell, f.tx, f.ty);
  // (as chief_ref_kernel: the rows re-read phase by phase, no apodization -- the chief ray's
  // intensity is not kept; of the flags only the pupil prescale, which (0, 0) does not feel)
  const Ray<double> g = opd_cell_ray<NR, false, true>(rows, n_surf, n_wl, f,
                                                      rg_flags & kRaygenPrescalePupil, 0.0, 0.0,
                                                      status);
  opd_cell_reference(w, g, cell->pupil_z);
  return w;
}

// ensemble_opd_kernel's body for one ray: OPD in waves against the cell's reference `ref` (read
// AFTER the walk, as opd_trace_kernel reads its own), the image-plane intensity, the point where
// the back-propagated ray meets the reference surface
template <int NR, bool APOD, bool FETCH>
OL_DEV void opd_cell_trace(const EnsembleRows<double>& rows, int n_surf, int n_wl,
                           const OpdCellField& f, uint32_t rg_flags,
                           cptr<WavefrontConsts<double>> ref, double px, double py,
                           uint32_t& status, double& opd_waves, double& intensity,
                           double (&pu)[3]) {
  Ray<double> g = opd_cell_ray<NR, APOD, FETCH>(rows, n_surf, n_wl, f, rg_flags, px, py, status);
  const WavefrontConsts<double> w = load_consts(refresh(ref));
  final_propagate<double, false>(w, g);
  opd_waves = wavefront_one<double>(w, g.x, g.y, g.z, g.L, g.M, g.N, g.opd, px, py, pu);
  intensity = g.i;
}

}  // namespace ol
