// forbes_device.h -- sag and sag gradient of the Forbes surfaces for ONE ray, and the Newton
// step on them: geometries/forbes/geometry.py (ForbesQNormalSlopeGeometry, ForbesQ2dGeometry)
// and geometries/forbes/qpoly.py as functions of the ray's own (x, y).  Used by
// forbes_trace_kernel (forbes.hip); under OL_HOST_MATH the same source runs on the host
// (tests/hostforbes), like the rest of the per-ray arithmetic.
//
// What the reference does per evaluation -- a Python Clenshaw loop per term list and per
// derivative order over arrays of alphas -- is here one backward sweep per term list in running
// registers: alpha^1_n needs only alpha^0_{n+1}, alpha^1_{n+1} and alpha^1_{n+2}, so value and
// derivative recurrences advance together and no alphas[] array exists (a runtime-indexed
// per-thread array would live in scratch).  The basis changes (change_basis_qbfs_to_pn,
// change_basis_q2d_to_pnm) and the recurrence constants A, B, C of every (n, m) are done once on
// the host, in fp64, when the table is packed; the sweeps read them wave-uniformly (scalar loads).
//
// The reference evaluates its sag and its normal at slightly DIFFERENT radial arguments, and the
// goldens hold both:
//   Q    sag     usq = r^2 / norm^2,                    departure cut for usq > 1
//        normal  u = sqrt(r^2 + 1e-24) / norm, usq = u^2, departure slope cut for u >= 1
//   Q2D  sag     u = sqrt(r^2 + 1e-12) / norm,          departure cut for u > 1
//        normal  u = sqrt(r^2) / norm,                  cut for u > 1; vertex case for rho < 1e-12
// so a sweep carries THREE recurrences: the value at the sag's argument, and the value and the
// derivative at the normal's.  Products round one by one (fp contract off), as the array
// expressions they restate.
//
// cos(m theta), sin(m theta) and u^m come from (x, y) / rho by the angle-addition recurrence and a
// running product instead of arctan2 / cos / sin / pow: they agree with the library calls to a few
// ulp times m (there is no argument reduction to go wrong: theta never exists), cost 6 products
// per order, and keep the library's table-driven slow paths -- private arrays -- out of the kernel.
//
// Device coefficient blocks (built by ol_system_create from the public ones, capi.hip;
// INTEGER slots hold bit patterns like the Zernike level headers):
//   kGeomForbesQ    [0] n0 (int)  [1] norm_radius  [2 ...] b_0 .. b_{n0-1}   (Pn basis)
//   kGeomForbesQ2d  [0] n0 (int)  [1] norm_radius  [2] M (int)  [3 ...] b_0 .. b_{n0-1},
//                   then for m = 1 .. M:  na (int), nb (int), na quads, nb quads; quad n of a
//                   list is (d_n, A_n, B_n, C_{n+1}): the Pnm-basis coefficient and the constants
//                   of   alpha_n = d_n + (A_n + B_n usq) alpha_{n+1} - C_{n+1} alpha_{n+2}
//                   (abc_q2d_clenshaw; C is 0 in the last two quads, where the reference has no
//                   such term)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_table.h"
#include "surface_math.h"

namespace ol {

// launch-uniform facts of the base conic, read where an evaluation starts
template <typename T>
struct ForbesBase {
  T R, k, kp1, cv;
  bool flat;   // |R| = inf
};

template <typename T>
OL_DEV ForbesBase<T> forbes_base(const DevSurf<T>& s) {
  return ForbesBase<T>{s.cold->radius, s.cold->conic, s.kp1, s.cv, (s.flags & kSurfRadiusInf) != 0};
}

// geometry.py:117-131 (_base_sag)
template <typename T>
OL_DEV T forbes_base_sag(const ForbesBase<T>& b, T r2) {
#pragma clang fp contract(off)
  using m = Math<T>;
  if (b.flat) return T(0);
  const T arg = T(1) - m::div(b.kp1 * r2, b.R * b.R);
  const T safe = arg < T(0) ? T(0) : arg;
  return m::div(r2, b.R * (T(1) + m::sqrt(safe)));
}

// geometry.py:133-149 (_base_sag_derivative)
template <typename T>
OL_DEV T forbes_base_slope(const ForbesBase<T>& b, T rho, T r2) {
#pragma clang fp contract(off)
  using m = Math<T>;
  if (b.flat || b.R == T(0)) return T(0);
  const T arg = T(1) - b.kp1 * (b.cv * b.cv) * r2;
  const T root = m::sqrt(arg > T(0) ? arg : T(1e-12));
  return m::div(b.cv * rho, root);
}

// geometry.py:151-181 (_conic_correction_factor): phi and d phi / d rho
template <typename T>
OL_DEV void forbes_conic_factor(const ForbesBase<T>& b, T r2, T& phi, T& dphi) {
#pragma clang fp contract(off)
  using m = Math<T>;
  if (b.flat) {
    phi = T(1);
    dphi = T(0);
    return;
  }
  const T c2 = b.cv * b.cv;
  const T rho = m::sqrt(r2);
  const T num = T(1) - b.k * c2 * r2, den = T(1) - b.kp1 * c2 * r2;
  const T N = m::sqrt(num > T(0) ? num : T(1e-12));
  const T D = m::sqrt(den > T(0) ? den : T(1e-12));
  phi = m::div(N, D);
  dphi = m::div(c2 * rho, N * (D * D * D));
}

// qpoly.py:131-143, 185-212, 265-283: the m = 0 list in the Pn basis.  S = 2 (alpha_0 + alpha_1)
// at usq_s (the sag's argument) and at usq, dS/dusq at usq.
template <typename T>
OL_DEV void forbes_sweep_m0(cptr<T> b, int n0, T usq_s, T usq, T& S_s, T& S, T& dS) {
#pragma clang fp contract(off)
  const T ps = T(2) - T(4) * usq_s, p = T(2) - T(4) * usq;
  T s1 = T(0), s2 = T(0), a1 = T(0), a2 = T(0), d1 = T(0), d2 = T(0);
  for (int n = n0 - 1; n >= 0; --n) {
    const T bn = b[n];
    const T sn = bn + ps * s1 - s2;
    const T an = bn + p * a1 - a2;
    const T dn = p * d1 - d2 - T(4) * a1;
    s2 = s1; s1 = sn;
    a2 = a1; a1 = an;
    d2 = d1; d1 = dn;
  }
  S_s = T(2) * (s1 + s2);
  S = T(2) * (a1 + a2);
  dS = T(2) * (d1 + d2);
}

// qpoly.py:507-536, 560-584, 403-412: one a- or b-list of azimuthal order m (quads, see above).
// The sum is alpha_0 / 2, for m = 1 with more than three coefficients minus 2/5 alpha_3, which
// is latched as the sweep passes it.
template <typename T>
OL_DEV void forbes_sweep_q2d(cptr<T> q, int n, bool m1, T usq_s, T usq, T& S_s, T& S, T& dS) {
#pragma clang fp contract(off)
  T s1 = T(0), s2 = T(0), a1 = T(0), a2 = T(0), d1 = T(0), d2 = T(0);
  T ls = T(0), la = T(0), ld = T(0);
  for (int k = n - 1; k >= 0; --k) {
    const T dk = q[4 * k], A = q[4 * k + 1], B = q[4 * k + 2], C = q[4 * k + 3];
    const T ws = A + B * usq_s, w = A + B * usq;
    const T sn = dk + ws * s1 - C * s2;
    const T an = dk + w * a1 - C * a2;
    const T dn = B * a1 + w * d1 - C * d2;
    s2 = s1; s1 = sn;
    a2 = a1; a1 = an;
    d2 = d1; d1 = dn;
    if (k == 3) {   // (wave-uniform)
      ls = sn;
      la = an;
      ld = dn;
    }
  }
  S_s = T(0.5) * s1;
  S = T(0.5) * a1;
  dS = T(0.5) * d1;
  if (m1 && n > 3) {
    const T f = T(2) / T(5);
    S_s = S_s - f * ls;
    S = S - f * la;
    dS = dS - f * ld;
  }
}

// ForbesQNormalSlopeGeometry.sag + _surface_normal_analytical (geometry.py:263-286, 311-369):
// sag and (d sag / dx, d sag / dy)
template <typename T>
OL_DEV void forbes_q_eval(const DevSurf<T>& s, cptr<T> c, T x, T y, T& sag, T& fx, T& fy) {
#pragma clang fp contract(off)
  using m = Math<T>;
  const ForbesBase<T> base = forbes_base(s);
  const int n0 = slot_int(c);
  const T norm = c[1];
  const T r2 = x * x + y * y;
  const T usq_s = m::div(r2, norm * norm);
  const T rho = m::sqrt(r2 + T(1e-24));
  const T u = m::div(rho, norm);
  const T usq = u * u;
  T S_s, S, dS;
  forbes_sweep_m0<T>(c + 2, n0, usq_s, usq, S_s, S, dS);
  T phi, dphi;
  forbes_conic_factor(base, r2, phi, dphi);
  const T dep = usq_s * (T(1) - usq_s) * phi * S_s;
  sag = forbes_base_sag(base, r2) + (usq_s > T(1) ? T(0) : dep);

  const T dS_du = dS * T(2) * u;                                 // qpoly.py:282
  const T dpre = m::div(T(2) * u - T(4) * (u * u * u), norm);
  const T dS_drho = m::div(dS_du, norm);
  const T pre = usq - usq * usq;
  const T slope = dpre * phi * S + pre * dphi * S + pre * phi * dS_drho;
  const T df = forbes_base_slope(base, rho, r2) + (u >= T(1) ? T(0) : slope);
  fx = df * m::div(x, rho);
  fy = df * m::div(y, rho);
}

// ForbesQ2dGeometry.sag + _surface_normal_analytical (geometry.py:539-571, 596-672) with
// compute_z_zprime_q2d / _compute_m_gt0_components (qpoly.py:422-473)
template <typename T>
OL_DEV void forbes_q2d_eval(const DevSurf<T>& s, cptr<T> c, T x, T y, T& sag, T& fx, T& fy) {
#pragma clang fp contract(off)
  using m = Math<T>;
  const ForbesBase<T> base = forbes_base(s);
  const int n0 = slot_int(c);
  const T norm = c[1];
  const int M = slot_int(c + 2);
  const T r2 = x * x + y * y;
  const T u_s = m::div(m::sqrt(r2 + T(1e-12)), norm);   // the sag's radial argument
  const T usq_s = u_s * u_s;
  const T rho = m::sqrt(r2);                            // the normal's
  const bool vertex = rho < T(1e-12);
  const T rho_safe = vertex ? T(1e-12) : rho;
  const T u = m::div(rho, norm);
  const T usq = u * u;
  // theta = arctan2(y, x) for both (safe_x is x: rho of the sag is never below 1e-6)
  const bool origin = !(rho > T(0));
  const T c1 = origin ? T(1) : m::div(x, rho), s1 = origin ? T(0) : m::div(y, rho);

  T S0_s, S0, dS0;
  forbes_sweep_m0<T>(c + 3, n0, usq_s, usq, S0_s, S0, dS0);
  cptr<T> p = c + 3 + n0;
  T sum_s = T(0), sum = T(0), dr = T(0), dt = T(0);   // the m > 0 sums
  T va = T(0), vb = T(0);                             // S_a, S_b of m = 1: the vertex gradient
  T cm = T(1), sm = T(0), um_s = T(1), um = T(1), umm1 = T(1);
  for (int mm = 1; mm <= M; ++mm) {
    const int na = slot_int(p), nb = slot_int(p + 1);
    T Sa_s, Sa, dSa, Sb_s, Sb, dSb;
    forbes_sweep_q2d<T>(p + 2, na, mm == 1, usq_s, usq, Sa_s, Sa, dSa);
    forbes_sweep_q2d<T>(p + 2 + 4 * na, nb, mm == 1, usq_s, usq, Sb_s, Sb, dSb);
    p += 2 + 4 * (na + nb);
    const T cn = cm * c1 - sm * s1, sn = sm * c1 + cm * s1;
    cm = cn;
    sm = sn;
    umm1 = um;
    um = um * u;
    um_s = um_s * u_s;
    const T fm = T(mm), two_usq = T(2) * usq;
    sum_s = sum_s + um_s * (cm * Sa_s + sm * Sb_s);
    sum = sum + um * (cm * Sa + sm * Sb);
    dr = dr + umm1 * (cm * (two_usq * dSa + fm * Sa) + sm * (two_usq * dSb + fm * Sb));
    dt = dt + fm * um * (-Sa * sm + Sb * cm);
    if (mm == 1) {
      va = Sa;
      vb = Sb;
    }
  }

  T phi, dphi;
  forbes_conic_factor(base, r2, phi, dphi);
  const T dep = usq_s * (T(1) - usq_s) * phi * S0_s + phi * sum_s;
  sag = forbes_base_sag(base, r2) + (u_s > T(1) ? T(0) : dep);

  const T dS0_drho = m::div(dS0 * T(2) * u, norm);
  const T dr_drho = m::div(dr, norm);
  const T dpre = m::div(T(2) * u - T(4) * (u * u * u), norm);
  const T pre = usq - usq * usq;
  const T ds0 = (dpre * S0 + pre * dS0_drho) * phi + pre * S0 * dphi;
  const T dsg = dphi * sum + phi * dr_drho;
  const bool cut = u > T(1);
  const T ds_drho = cut ? T(0) : ds0 + dsg;
  const T ds_dth = cut ? T(0) : phi * dt;
  const T ct = m::div(x, rho_safe), st = m::div(y, rho_safe);
  const T db = forbes_base_slope(base, rho, r2);
  const T gx = db * ct + (ct * ds_drho - m::div(st, rho_safe) * ds_dth);
  const T gy = db * st + (st * ds_drho + m::div(ct, rho_safe) * ds_dth);
  fx = vertex ? m::div(va, norm) : gx;
  fy = vertex ? m::div(vb, norm) : gy;
}

template <typename T>
OL_DEV void forbes_eval(const DevSurf<T>& s, cptr<T> c, T x, T y, T& sag, T& fx, T& fy) {
  if (s.geom == kGeomForbesQ2d) forbes_q2d_eval(s, c, x, y, sag, fx, fy);
  else forbes_q_eval(s, c, x, y, sag, fx, fy);
}

// The Newton start: the reference's own intersection with the base conic (standard.py:97-148)
// in ITS form and in IEEE operations -- plain quotients and square roots, nothing contracted --
// and the start point as x + t L rounded product by product.  Not for accuracy: the Q2D sag of
// the reference is double-valued at the vertex (its radial argument never falls below
// 1e-6 / norm_radius, so the m = 1 terms leave a step of ~1e-10 mm across rho = 0 whose side is
// sin(theta), cos(theta)), and a ray aimed at the vertex -- every chief ray when the stop is on the
// surface -- has a root on either side.  Which one the reference's iteration finds is decided by
// the SIGN of the rounding noise (~1e-16) of its first point; the same operations in the same
// order give the same bits, hence the same side.
OL_DEV double forbes_ieee_sqrt(double v) { return __builtin_sqrt(v); }
OL_DEV float forbes_ieee_sqrt(float v) { return __builtin_sqrtf(v); }

template <typename T>
OL_DEV T forbes_start_distance(const DevSurf<T>& s, T x, T y, T z, T L, T M, T N) {
#pragma clang fp contract(off)
  if (s.flags & kSurfRadiusInf) {
    const T Ns = __builtin_fabs((double)N) > 1e-14 ? N : T(1e-14);
    return -z / Ns;
  }
  const T R = s.cold->radius, k = s.cold->conic;
  const T NN = N * N, zz = z * z;
  const T a = ((k * NN + L * L) + M * M) + NN;
  const T b = (((((T(2) * k) * N) * z + (T(2) * L) * x) + (T(2) * M) * y) - (T(2) * N) * R) +
              (T(2) * N) * z;
  const T c = (((k * zz - (T(2) * R) * z) + x * x) + y * y) + zz;
  const T d = b * b - (T(4) * a) * c;
  const T sq = forbes_ieee_sqrt(d);   // NaN when the ray misses the base conic
  const T t1 = (-b + sq) / (T(2) * a), t2 = (-b - sq) / (T(2) * a);
  const T z1 = z + t1 * N, z2 = z + t2 * N;
  T t = Math<T>::abs(z1) <= Math<T>::abs(z2) ? t1 : t2;
  if (a == T(0)) t = -c / b;
  return t;
}

// One Newton update on a Forbes surface: newton_iterate (surface_math.h) with this file's
// functors -- the re-based iteration, the per-ray stop rule and the rounding-floor exit are the
// project's for every Newton geometry (newton_raphson.py:119-168 stops batch-wide).
template <typename T>
OL_DEV void forbes_newton_iterate(const DevSurf<T>& s, cptr<T> c, NewtonRay<T>& q, T L, T M, T N,
                                  int it) {
  using m = Math<T>;
  const T xi = m::fma(q.dt, L, q.xb), yi = m::fma(q.dt, M, q.yb), zi = m::fma(q.dt, N, q.zb);
  T sag, fx, fy;
  forbes_eval(s, c, xi, yi, sag, fx, fy);
  const T f = sag - zi;
  const T af = m::abs(f);
  bool done = !(af >= s.cold->tol);   // converged, or NaN
  const bool at_floor = !(af > T(OL_NR_STALL_ULPS) * m::eps() * (m::abs(sag) + m::abs(zi)));
  done = done || (it > 0 && at_floor && !(af < T(0.5) * q.fprev));
  const T df = m::fma(fx, L, m::fma(fy, M, -N));
  const T dfs = m::abs(df) > m::guard() ? df : m::guard();
  q.dt = q.dt - m::div(f, dfs);
  q.fprev = af;
  q.gx = fx;
  q.gy = fy;
  q.active = !done;
}

// The Forbes row of Surface._trace_real (surfaces/standard_surface.py:232-258) for one ray that
// is in the GLOBAL frame: into the surface's frame, the Newton solve from the base conic's hit,
// the interaction (propagation, absorption, OPD, clip, Snell / reflection, simple coating:
// interact<>, unpolarised), back to the global frame.
template <typename T, typename H>
OL_DEV Ray<T> forbes_step(const H& h, cptr<T> coeffs, Ray<T> ray) {
  using m = Math<T>;
  Ray<T> r[1] = {ray};
  into_local_frame<T, 1>(h.surf(), true, r);
  NewtonRay<T> q;
  T t[1];
  int max_iter;
  {
    const DevSurf<T> s = h.surf();
    max_iter = s.max_iter;
    t[0] = forbes_start_distance<T>(s, r[0].x, r[0].y, r[0].z, r[0].L, r[0].M, r[0].N);
    {
#pragma clang fp contract(off)
      q.xb = r[0].x + t[0] * r[0].L;   // (newton_raphson.py:139-141)
      q.yb = r[0].y + t[0] * r[0].M;
      q.zb = r[0].z + t[0] * r[0].N;
    }
    q.dt = q.fprev = q.gx = q.gy = T(0);
    q.active = true;
  }
  int it = 0;
  for (; it < max_iter; ++it) {
    const DevSurf<T> s = h.surf();
    if (q.active) forbes_newton_iterate<T>(s, coeffs + s.coeff_off, q, r[0].L, r[0].M, r[0].N, it);
    if (!hw::wave_any(q.active)) {
      ++it;
      break;
    }
  }
  r[0].x = m::fma(q.dt, r[0].L, q.xb);
  r[0].y = m::fma(q.dt, r[0].M, q.yb);
  r[0].z = m::fma(q.dt, r[0].N, q.zb);
  t[0] = t[0] + q.dt;
  {
    // the normal AT the end point, as Surface._trace_real takes it (standard_surface.py:246-250),
    // not the last iterate's as the fused kernels do: near the vertex of a Q2D surface the
    // gradient holds (d sag / d theta) / rho, which moves by 1e-13 over a last step of 1e-12 mm --
    // half the tight bound -- and one more evaluation per ray is a fifth of the solve
    const DevSurf<T> s = h.surf();
    T sag;
    forbes_eval(s, coeffs + s.coeff_off, r[0].x, r[0].y, sag, q.gx, q.gy);
  }
  const T im = m::rsqrt(m::fma(q.gx, q.gx, m::fma(q.gy, q.gy, T(1))));
  const T nx[1] = {q.gx * im}, ny[1] = {q.gy * im}, nz[1] = {-im};
  Prt<T, 0> P[1];
  bool prt_fresh = false;
  {
    const DevSurf<T> s = h.surf();
    const DevOptics<T> o = h.optics();
    interact<T, 1, 0, true>(s, o, coeffs, t, nx, ny, nz, r, P, prt_fresh);
  }
  return to_global<T>(h.surf(), r[0]);
}

}  // namespace ol
