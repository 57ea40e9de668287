// ray_aim_device.h -- iterative ray aiming for ONE ray: the Broyden solve of
// rays/ray_aiming/iterative.py:136-281 as a function of the ray's own state.  Used by
// aim_rays_kernel (ray_aim.hip); under OL_HOST_MATH the same source runs on the host
// (tests/hostaim), like the rest of the per-ray arithmetic.
//
// The reference solves a whole batch at once, but nothing couples its rays: each carries its own
// 2 x 2 Jacobian estimate, error and active flag, and a converged ray is traced again every pass
// only because the batch is.  What IS batch-global -- the early return, the two ValueErrors -- is
// left to the host as two status bits.
//
// Control flow is wave-uniform: every lane evaluates every pass until no lane of the wave is
// active, and a converged lane merely does not commit (surface_step's Newton loops vote across
// the wave; a lane that left early would change nothing but leaves nothing to gain either).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_table.h"
#include "surface_math.h"

namespace ol {

constexpr uint32_t kAimNanGuess = 0x100u;      // OL_AIM_NAN_GUESS
constexpr uint32_t kAimNotConverged = 0x200u;  // OL_AIM_NOT_CONVERGED

// launch-uniform scalars of the solve (ol_aim_params without the generator block)
struct AimConsts {
  double r_stop, jacobian, tol;
  int32_t max_iter, infinite;
};

// the fp64 surface table and the traced range [first, stop]
struct AimTable {
  const DevSurfHot<double>* surf;
  const DevSurfCold<double>* cold;
  const DevOptics<double>* optics;
  const double* coeffs;
  int32_t first, stop, n_wl, wl;
};

OL_DEV SurfFetched<double> aim_surface(const AimTable& t, int s) {
  return SurfFetched<double>{as_const(t.surf) + s, as_const(t.cold) + s,
                             as_const(t.optics) + (s * t.n_wl + t.wl)};
}

// iterative.py:339-367 + :309-337: a copy of the launch state through surfaces [first, stop]
// (unpolarised; the intensity is carried and never read), then its position in the stop
// surface's own frame.  The reference goes through the global frame after every surface; the
// kernels carry a ray from frame to frame (into_local_frame), so after the stop surface's step
// the state IS stop-local.  Only a stop that does not interact (record-only) is reached through
// the global frame.
template <int NR>
OL_DEV void aim_evaluate(const AimTable& t, const double (&o)[6], double& lx, double& ly,
                         uint32_t& status) {
  Ray<double> r[1];
  r[0].x = o[0]; r[0].y = o[1]; r[0].z = o[2];
  r[0].L = o[3]; r[0].M = o[4]; r[0].N = o[5];
  r[0].i = 1.0;
  r[0].opd = 0.0;
  Prt<double, 0> P[1];
  bool is_global = true, prt_fresh = false;
  int last = t.first;
  for (int s = t.first; s <= t.stop; ++s) {
    const SurfFetched<double> h = aim_surface(t, s);
    if (refresh(h.hot)->interaction != kRecordOnly) {
      surface_step<double, 1, 0, NR>(h, as_const(t.coeffs), is_global, r, P, status, prt_fresh);
      is_global = false;
      last = s;
    }
  }
  if (is_global || last != t.stop) {
    if (!is_global) r[0] = to_global<double>(aim_surface(t, last).surf(), r[0]);
    into_local_frame<double, 1>(aim_surface(t, t.stop).surf(), true, r);
  }
  lx = r[0].x;
  ly = r[0].y;
}

// o[0..5] = x, y, z, L, M, N: the start on entry, the solution on return.  (px, py): the
// normalised pupil point the ray is aimed at.  `updates`: how many passes moved this ray.
// Returns the ray's kAim* bits (+ whatever surface_step reports in `status`).
template <int NR>
OL_DEV uint32_t aim_one(const AimTable& t, const AimConsts& c, double px, double py,
                        double (&o)[6], int32_t& updates, uint32_t& status) {
// the solver's own arithmetic rounds product by product, like the array expressions it restates
#pragma clang fp contract(off)
  const double tx = px * c.r_stop, ty = py * c.r_stop;   // iterative.py:127-132
  const double tol2 = c.tol * c.tol;
  const int a = c.infinite ? 0 : 3;   // the unknowns: (x, y) or (L, M); N is NOT renormalised
  uint32_t bits = 0;
  double lx, ly;
  aim_evaluate<NR>(t, o, lx, ly, status);
  double ex = lx - tx, ey = ly - ty;
  if (ex != ex) bits |= kAimNanGuess;   // :141-145 (the reference looks at ex alone)
  const double jf = fabs(c.jacobian) < 1e-12 ? 1e-12 : c.jacobian;   // :154-156
  double J11 = jf, J12 = 0.0, J21 = 0.0, J22 = jf;
  updates = 0;
  for (int it = 0; it < c.max_iter; ++it) {
    const bool active = !(ex * ex + ey * ey < tol2);   // :185-192 (a NaN error stays active)
    if (!hw::wave_any(active)) break;                  // :188: every ray of the wave converged
    double det = J11 * J22 - J12 * J21;
    det = fabs(det) < 1e-12 ? 1e-12 : det;             // :211
    const double dp1 = -(J22 * ex + (-J12) * ey) / det;   // :214-220
    const double dp2 = -((-J21) * ex + J11 * ey) / det;
    double q[6] = {o[0], o[1], o[2], o[3], o[4], o[5]};
    q[a] += dp1;
    q[a + 1] += dp2;
    aim_evaluate<NR>(t, q, lx, ly, status);
    const double exn = lx - tx, eyn = ly - ty;
    // Broyden: J += (dE - J s) s^T / max(|s|^2, 1e-20), with the OLD J (:243-272)
    const double Rx = (exn - ex) - (J11 * dp1 + J12 * dp2);
    const double Ry = (eyn - ey) - (J21 * dp1 + J22 * dp2);
    double norm = dp1 * dp1 + dp2 * dp2;
    norm = norm < 1e-20 ? 1e-20 : norm;   // (be.maximum: a NaN stays one)
    if (active) {
      o[a] = q[a];
      o[a + 1] = q[a + 1];
      J11 += Rx * dp1 / norm;
      J12 += Rx * dp2 / norm;
      J21 += Ry * dp1 / norm;
      J22 += Ry * dp2 / norm;
      ex = exn;
      ey = eyn;
      ++updates;
    }
  }
  if (!(ex * ex + ey * ey < tol2)) bits |= kAimNotConverged;   // :278-279
  return bits;
}

}  // namespace ol
