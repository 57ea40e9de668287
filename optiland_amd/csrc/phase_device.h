// phase_device.h -- a phase-profile plane for ONE ray: Surface._trace_real
// (surfaces/standard_surface.py:232-258) on a Plane with PhaseInteractionModel
// (interactions/phase_interaction_model.py:45-132) and the profiles of optiland/phase/ --
// constant.py, linear_grating.py, radial.py, grid.py, height_profile.py.  Used by
// phase_trace_kernel (phase.hip); under OL_HOST_MATH the same source runs on the host
// (tests/hostphase).
//
// The model is the generalised law of refraction on a plane whose normal is (0, 0, 1): the
// tangential wave vector gains the gradient of the phase.  With k0 = 2 pi / (wavelength * 1e-3)
// divided out -- q = 1 / k0 = wavelength_um * 1e-3 / (2 pi), formed on the host in double --
//   p   = q scale phi(x, y)              (gx, gy) = q scale grad phi(x, y)
//   n2' = n1 if reflecting else n2
//   tx  = n1 L + gx     ty = n1 M + gy   (the z part of the tangential vector is n1 N - n1 N = 0)
//   S   = n2'^2 - tx^2 - ty^2            S < 0: intensity 0 and S = 0 (rays.clip, maximum(0, .));
//                                        a NaN compares false and stays NaN
//   kz  = -sqrt(S) if reflecting else +sqrt(S)     whatever the sign of the incoming N
//   (L, M, N) = (tx, ty, kz) / |(tx, ty, kz)|      opd -= p
// then SimpleCoating, then intensity *= efficiency.  Checked against the reference's NumPy and
// torch backends in fp64: directions to 2.2e-16.
//
// Radial: phi = sum a_2p r^2p and d phi / d(x, y) = g(r^2) (x, y), g = sum 2p a_2p r^(2p-2), both
// by Horner in r^2 over the term list, highest term first, in running registers.  The reference
// forms d phi / dr / r with a branch at r = 0; g (x, y) is that number to rounding and 0 at r = 0.
//
// Grid (GridPhaseProfile, HeightProfile): what the reference's TORCH backend computes
// (phase/interpolators.py:72-121) -- grid_sample(mode="bilinear", align_corners=True,
// padding_mode="zeros") and its derivative:
//   ix = ((2 (x - xmin) / (xmax - xmin) - 1) + 1) / 2 * (W - 1), iy likewise; x0 = floor(ix);
//   value = sum of the four neighbours times (x0 + 1 - ix | ix - x0)(y0 + 1 - iy | iy - y0), a
//   neighbour outside the grid counting as 0;
//   d/dx = ((v01 - v00)(y0 + 1 - iy) + (v11 - v10)(iy - y0)) (W - 1) / (xmax - xmin), d/dy likewise.
// Only the end points of the coordinate vectors enter, as there.  The four loads are the only
// indexed memory access: every index is clamped into the grid BEFORE the load (in floating point,
// where a NaN clamps to 0, then converted) and the value is masked AFTER it, so no lane reads
// outside the block whatever its ray is; a NaN position gives NaN weights and a NaN result.
// The NumPy backend's SciPy spline is another interpolant and is not reproduced.
//
// Device coefficient block (built by ol_system_create from the public one, capi.hip); (i): an
// integer bit pattern, a scalar-unit operand:
//   [0] profile kind (i)  [1] efficiency
//   constant  [2] phase
//   linear    [2] K_x  [3] K_y
//   radial    [2] count (i), then a_2, a_4, ...
//   grid      [2] W (i)  [3] H (i)  [4] xmin  [5] xmax - xmin  [6] ymin  [7] ymax - ymin
//             [8] W - 1  [9] H - 1  [10] (W - 1) / (xmax - xmin)  [11] (H - 1) / (ymax - ymin)
//             [12] n_scale (i), then n_scale scales, then H * W node values, row-major
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_table.h"
#include "surface_math.h"

namespace ol {

OL_DEV float phase_floor(float v) { return __builtin_floorf(v); }
OL_DEV double phase_floor(double v) { return __builtin_floor(v); }
// v into [0, hi] as an index; a NaN becomes 0 (fmax / fmin return the operand that is a number)
OL_DEV int32_t phase_index(float v, float hi) {
  return (int32_t)__builtin_fminf(__builtin_fmaxf(v, 0.0f), hi);
}
OL_DEV int32_t phase_index(double v, double hi) {
  return (int32_t)__builtin_fmin(__builtin_fmax(v, 0.0), hi);
}

// phi and its gradient at (x, y), both times `scale` of the block (1 without scales).
// c: the surface's block; nodes: the same block as a GLOBAL pointer, for the per-lane gathers.
template <typename T>
OL_DEV void phase_profile(cptr<T> c, const T* nodes, int32_t wl, T x, T y, T& phi, T& gx, T& gy) {
  using m = Math<T>;
  const int32_t kind = slot_int(c);
  if (kind == kPhaseConstant) {
    phi = c[2];
    gx = gy = T(0);
  } else if (kind == kPhaseLinear) {
    const T kx = c[2], ky = c[3];
    phi = m::fma(kx, x, ky * y);
    gx = kx;
    gy = ky;
  } else if (kind == kPhaseRadial) {
    const int32_t count = slot_int(c + 2);
    const T r2 = m::fma(x, x, y * y);
    T f = T(0), g = T(0);
    for (int32_t k = count - 1; k >= 0; --k) {
      const T a = c[3 + k];
      f = m::fma(f, r2, a);
      g = m::fma(g, r2, T(2 * (k + 1)) * a);
    }
    phi = f * r2;
    gx = g * x;
    gy = g * y;
  } else {
    const int32_t W = slot_int(c + 2), n_scale = slot_int(c + 12);
    const T wm1 = c[8], hm1 = c[9];
    const T ix = (((T(2) * m::div(x - c[4], c[5]) - T(1)) + T(1)) * T(0.5)) * wm1;
    const T iy = (((T(2) * m::div(y - c[6], c[7]) - T(1)) + T(1)) * T(0.5)) * hm1;
    const T fx = phase_floor(ix), fy = phase_floor(iy);
    const T fx1 = fx + T(1), fy1 = fy + T(1);
    // a neighbour outside the grid counts as 0 (a NaN compares false: masked, weights NaN)
    const bool inx0 = fx >= T(0) && fx <= wm1, inx1 = fx1 >= T(0) && fx1 <= wm1;
    const bool iny0 = fy >= T(0) && fy <= hm1, iny1 = fy1 >= T(0) && fy1 <= hm1;
    const int32_t x0 = phase_index(fx, wm1), x1 = phase_index(fx1, wm1);
    const int32_t y0 = phase_index(fy, hm1), y1 = phase_index(fy1, hm1);
    const T* v = nodes + kPhaseGridHead + n_scale;
    const T l00 = v[y0 * W + x0], l01 = v[y0 * W + x1];
    const T l10 = v[y1 * W + x0], l11 = v[y1 * W + x1];
    const T v00 = (inx0 && iny0) ? l00 : T(0), v01 = (inx1 && iny0) ? l01 : T(0);
    const T v10 = (inx0 && iny1) ? l10 : T(0), v11 = (inx1 && iny1) ? l11 : T(0);
    const T ax = fx1 - ix, bx = ix - fx, ay = fy1 - iy, by = iy - fy;
    const T scale = n_scale > 0 ? c[kPhaseGridHead + wl] : T(1);
    phi = scale * m::fma(v00 * ax, ay, m::fma(v01 * bx, ay, m::fma(v10 * ax, by, (v11 * bx) * by)));
    gx = scale * (m::fma(v01 - v00, ay, (v11 - v10) * by) * c[10]);
    gy = scale * (m::fma(v10 - v00, ax, (v11 - v01) * bx) * c[11]);
  }
}

// The phase row of Surface._trace_real for one ray that is in the GLOBAL frame: into the
// surface's frame, the plane hit, propagation, absorption, OPD and clip (the steps of interact<>,
// surface_math.h, in its order and words), the interaction above, a simple coating, the
// efficiency, back to the global frame.  Unpolarised.  q: wavelength_um * 1e-3 / (2 pi).
template <typename T, typename H>
OL_DEV Ray<T> phase_step(const H& h, cptr<T> coeffs, const T* coeffs_global, Ray<T> ray,
                         int32_t wl, T q) {
  using m = Math<T>;
  Ray<T> r[1] = {ray};
  into_local_frame<T, 1>(h.surf(), true, r);
  const DevSurf<T> s = h.surf();
  const DevOptics<T> o = h.optics();
  cptr<T> c = coeffs + s.coeff_off;
  // geometries/plane.py: t = -z / N
  const T t = -m::div(r[0].z, r[0].N);
  r[0].x = m::fma(t, r[0].L, r[0].x);
  r[0].y = m::fma(t, r[0].M, r[0].y);
  r[0].z = m::fma(t, r[0].N, r[0].z);
  // homogeneous.py:44-53 (see interact<> for the clipped-ray case)
  if (o.absorb > T(0)) {
    const T arg = -o.absorb * t;
    const T prod = r[0].i * m::exp(arg);
    r[0].i = (r[0].i == T(0) && arg < T(709.78)) ? T(0) : prod;
  }
  r[0].opd = r[0].opd + m::abs(t * o.n1);
  if (s.aperture_kind != kApNone)
    r[0].i = aperture_contains<T, true>(s, coeffs, r[0].x, r[0].y) ? r[0].i : T(0);
  T phi, gx, gy;
  phase_profile<T>(c, coeffs_global + s.coeff_off, wl, r[0].x, r[0].y, phi, gx, gy);
  const bool reflect = s.interaction == kReflect;
  const T n1 = o.n1, n2 = reflect ? o.n1 : o.n2;
  const T tx = m::fma(n1, r[0].L, q * gx), ty = m::fma(n1, r[0].M, q * gy);
  T S = m::fma(n2, n2, -m::fma(tx, tx, ty * ty));
  if (S < T(0)) {   // evanescent: clipped, and the ray goes on along the surface
    r[0].i = T(0);
    S = T(0);
  }
  const T kz = reflect ? -m::sqrt(S) : m::sqrt(S);
  const T ik = m::rsqrt(m::fma(tx, tx, m::fma(ty, ty, kz * kz)));
  r[0].L = tx * ik;
  r[0].M = ty * ik;
  r[0].N = kz * ik;
  r[0].opd = m::fma(-q, phi, r[0].opd);
  // coating (interactions/base.py:111-128), then the profile's efficiency
  if (s.coating_kind == kCoatSimple)
    r[0].i = r[0].i * (reflect ? s.cold->coat[1] : s.cold->coat[0]);
  r[0].i = r[0].i * c[1];
  return to_global<T>(s, r[0]);
}

}  // namespace ol
