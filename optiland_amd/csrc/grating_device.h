// grating_device.h -- a diffraction grating for ONE ray: the grating row of Surface._trace_real
// (surfaces/standard_surface.py:232-258) on PlaneGrating / StandardGratingGeometry
// (geometries/plane_grating.py, geometries/standard_grating.py) with
// DiffractiveInteractionModel (interactions/diffractive_model.py:28-61) and
// RealRays.gratingdiffract (rays/real_rays.py:207-522).  Used by grating_trace_kernel
// (grating.hip); under OL_HOST_MATH the same source runs on the host (tests/hostgrating).
//
// The reference's gratingdiffract is some 150 lines of expanded polynomial per direction
// component.  Collected, it is the tangential-momentum form below (checked against the
// reference's NumPy backend: 2-3e-16 on random rays, both geometries, both interactions):
//   n      unit normal, aligned with the ray as _align_surface_normal does: n_raw * sign(k0.n_raw),
//          sign(0) = 0;  c = |k0 . n_raw|
//   f      grating vector.  Plane: (-sin a, cos a, 0).  Standard: -(n_raw x t) / |n_raw x t| with
//          t = (1, tan a, dz/dx|_groove) (standard_grating.py:102-155), n_raw NOT aligned
//   d_eff  period / sqrt(fx^2 + fy^2)                  (diffractive_model.py:51)
//   g      order * wavelength / d_eff                  (wavelength and period in micrometres)
//   T      n1 (k0 - c n) + g (f - (f.n) n)             the tangential part behind the surface
//   S      n2^2 - |T|^2                                < 0: evanescent order, direction NaN
//   k1     normalize(( T + sigma n sqrt(S)) / n2)      refracting
//          normalize((-T + sigma n sqrt(S)) / n2)      reflecting -- what the reference's formula
//          evaluates to with its n2c = -n2 and its -n sqrt(S) term; NOT the textbook mirror
//          direction.  The reference's numbers are the contract.
//   sigma  sign(period): the reference's root is sqrt(d^2 S) = |d| sqrt(S) over d n2, so a
//          NEGATIVE period flips the normal term (period -5 with order +1 is not period +5 with
//          order -1 there: the ray leaves on the other side of the surface)
// At exactly k0 . n_raw = 0 the reference's aligned normal is the zero vector, its numerators
// vanish and normalize() divides 0 by 0: NaN.  Here sign(0)^2 = 0 scales the direction before the
// normalisation to the same end.
// The hit point stays finite when the direction is NaN, as in the reference.
//
// StandardGratingGeometry._tangent writes d sag / dx along the groove as
//   (x + y tan a) (2 R^2 s (s + 1) + (k + 1) r^2) / (R^3 s (s + 1)^2),  s = sqrt(1 - (k + 1) r^2 / R^2).
// With (k + 1) r^2 / R^2 = 1 - s^2 the bracket is R^2 (s + 1)^2, so the quotient is
// (x + y tan a) / (R s): the same number to rounding, one square root and one quotient.  The
// tangent's own normalisation drops out of f, which is normalised after the cross product.
//
// Device coefficient block (built by ol_system_create from the public one, capi.hip):
//   [0] order  [1] period (um)  [2] sin a  [3] cos a  [4] tan a        a: groove orientation angle
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_table.h"
#include "surface_math.h"

namespace ol {

constexpr int kGratingBlock = 5;   // values of the device coefficient block

// Intersection and RAW (un-aligned) unit normal; the ray is moved to the hit.  Plane:
// plane_grating.py:74-111 (t = -z / N, normal (0, 0, 1)).  Standard: the conic intersection of
// the kGeomStandard rows (surface_math.h; kSurfReferenceRoot: the reference's own quadratic) and
// standard_grating.py:206-231.
template <typename T>
OL_DEV T grating_hit(const DevSurf<T>& s, Ray<T>& r, T& nx, T& ny, T& nz, T& slope) {
  using m = Math<T>;
  T t;
  if (s.geom == kGeomPlaneGrating) {
    t = -m::div(r.z, r.N);
    r.x = m::fma(t, r.L, r.x);
    r.y = m::fma(t, r.M, r.y);
    r.z = m::fma(t, r.N, r.z);
    nx = ny = T(0);
    nz = T(1);
    slope = T(0);
    return t;
  }
  const T cv = s.cv, kp1 = s.kp1;
  if (s.flags & kSurfReferenceRoot)
    t = reference_distance<T>(s.cold->radius, s.cold->conic, r.x, r.y, r.z, r.L, r.M, r.N);
  else
    t = curved_distance<T>(cv, kp1, r.x, r.y, r.z, r.L, r.M, r.N);
  r.x = m::fma(t, r.L, r.x);
  r.y = m::fma(t, r.M, r.y);
  r.z = m::fma(t, r.N, r.z);
  // (fx, fy) = cv (x, y) / s,  s = sqrt(1 - (1 + k) cv^2 r^2): NaN beyond the conic's rim
  const T r2 = m::fma(r.x, r.x, r.y * r.y);
  const T is = m::rsqrt(m::fma(-kp1 * cv * cv, r2, T(1)));
  slope = cv * is;
  const T fx = r.x * slope, fy = r.y * slope;
  const T im = m::rsqrt(m::fma(fx, fx, m::fma(fy, fy, T(1))));
  nx = fx * im;
  ny = fy * im;
  nz = -im;
  return t;
}

// RealRays.gratingdiffract with the grating vector and the period correction of
// DiffractiveInteractionModel.interact_real_rays: the direction behind the surface, normalised.
// (nx, ny, nz): the RAW normal at the hit; slope: cv / s of grating_hit (standard geometry);
// gq = order * wavelength / period.
template <typename T>
OL_DEV void grating_diffract(const DevSurf<T>& s, const DevOptics<T>& o, cptr<T> c, T gq, T slope,
                             T nx, T ny, T nz, Ray<T>& r) {
  using m = Math<T>;
  const T L0 = r.L, M0 = r.M, N0 = r.N;
  T fx, fy, fz;
  if (s.geom == kGeomPlaneGrating) {
    fx = -c[2];
    fy = c[3];
    fz = T(0);
  } else {
    const T ta = c[4];
    const T tz = m::fma(r.y, ta, r.x) * slope;   // t = (1, tan a, tz), not normalised
    const T cx = m::fma(ny, tz, -nz * ta), cy = m::fma(-nx, tz, nz), cz = m::fma(nx, ta, -ny);
    const T ic = -m::rsqrt(m::fma(cx, cx, m::fma(cy, cy, cz * cz)));
    fx = cx * ic;
    fy = cy * ic;
    fz = cz * ic;
  }
  const T g = gq * m::sqrt(m::fma(fx, fx, fy * fy));
  const T dot = m::fma(L0, nx, m::fma(M0, ny, N0 * nz));
  // be.sign(dot): +-1, 0 at 0, NaN for NaN
  const T sgn = dot != T(0) ? m::copysign(T(1), dot) : T(0);
  const T ax = nx * sgn, ay = ny * sgn, az = nz * sgn;
  const T fn = m::fma(fx, nx, m::fma(fy, ny, fz * nz));
  // T = n1 (k0 - dot n_raw) + g (f - (f.n) n): for sgn = +-1 both brackets do not see the
  // alignment (sgn = 0: see below)
  const T n1 = o.n1, n2 = o.n2;
  const T tx = m::fma(n1, m::fma(-dot, nx, L0), g * m::fma(-fn, nx, fx));
  const T ty = m::fma(n1, m::fma(-dot, ny, M0), g * m::fma(-fn, ny, fy));
  const T tz = m::fma(n1, m::fma(-dot, nz, N0), g * m::fma(-fn, nz, fz));
  const T S = m::fma(n2, n2, -m::fma(tx, tx, m::fma(ty, ty, tz * tz)));
  const T root = m::copysign(m::sqrt(S), c[1]);   // NaN: evanescent order; sign(period)
  const T ts = s.interaction == kReflect ? T(-1) : T(1);
  // sgn^2: 1, or 0 at exactly grazing incidence, where the reference ends in 0 / 0
  const T s2 = sgn * sgn;
  const T kx = s2 * m::fma(ts, tx, ax * root), ky = s2 * m::fma(ts, ty, ay * root),
          kz = s2 * m::fma(ts, tz, az * root);
  // (the quotient by n2 drops out of the normalisation: n2 > 0)
  const T ik = m::rsqrt(m::fma(kx, kx, m::fma(ky, ky, kz * kz)));
  r.L = kx * ik;
  r.M = ky * ik;
  r.N = kz * ik;
}

// The grating row of Surface._trace_real for one ray that is in the GLOBAL frame: into the
// surface's frame, the intersection, propagation, absorption, OPD and clip (the steps of
// interact<>, surface_math.h, in its order and words), the diffraction, a simple coating, back to
// the global frame.  Unpolarised.  wavelength: micrometres.
template <typename T, typename H>
OL_DEV Ray<T> grating_step(const H& h, cptr<T> coeffs, Ray<T> ray, T wavelength) {
  using m = Math<T>;
  Ray<T> r[1] = {ray};
  into_local_frame<T, 1>(h.surf(), true, r);
  const DevSurf<T> s = h.surf();
  const DevOptics<T> o = h.optics();
  cptr<T> c = coeffs + s.coeff_off;
  T nx, ny, nz, slope;
  const T t = grating_hit<T>(s, r[0], nx, ny, nz, slope);
  // homogeneous.py:44-53 (see interact<> for the clipped-ray case)
  if (o.absorb > T(0)) {
    const T arg = -o.absorb * t;
    const T prod = r[0].i * m::exp(arg);
    r[0].i = (r[0].i == T(0) && arg < T(709.78)) ? T(0) : prod;
  }
  r[0].opd = r[0].opd + m::abs(t * o.n1);
  if (s.aperture_kind != kApNone)
    r[0].i = aperture_contains<T, true>(s, coeffs, r[0].x, r[0].y) ? r[0].i : T(0);
  const T gq = m::div(c[0] * wavelength, c[1]);
  grating_diffract<T>(s, o, c, gq, slope, nx, ny, nz, r[0]);
  // coating (interactions/base.py:111-128)
  if (s.coating_kind == kCoatSimple)
    r[0].i = r[0].i * (s.interaction == kReflect ? s.cold->coat[1] : s.cold->coat[0]);
  return to_global<T>(s, r[0]);
}

}  // namespace ol
