// grid_sag_device.h -- a grid-sag surface for ONE ray: Surface._trace_real
// (surfaces/standard_surface.py:232-258) on GridSagGeometry (geometries/grid_sag.py), the
// reference's geometry for measured and freeform surfaces.  Used by grid_sag_trace_kernel
// (grid_sag.hip); under OL_HOST_MATH the same source runs on the host (tests/hostgrid).
//
// The sag is the bilinear interpolant of a table z[j][i] over two strictly increasing coordinate
// vectors x_0 .. x_{W-1}, y_0 .. y_{H-1}, which need not be uniform (grid_sag.py:61-101):
//   i = searchsorted(x_grid, x, side="right") - 1, clamped to [0, W - 2]; j likewise
//   tx = (x - x_i) / (x_{i+1} - x_i)                 ty likewise
//   sag   = (z11 (1 - tx) + z12 tx) (1 - ty) + (z21 (1 - tx) + z22 tx) ty
//   ds/dx = ((z12 - z11) (1 - ty) + (z22 - z21) ty) / (x_{i+1} - x_i)
//   ds/dy = ((z21 - z11) (1 - tx) + (z22 - z12) tx) / (y_{j+1} - y_j)
//   sag = NaN outside [x_0, x_{W-1}] x [y_0, y_{H-1}]
// in the reference's own order of operations, products rounded one by one (fp contract off).
//
// The cell is the reference's for every finite point, taken from the STORED coordinates: a ray
// through a node (the chief ray at x = 0) or along a cell border must land in the cell the
// reference takes, since the slope -- and so the normal -- differs across the border.  Cell i
// holds x exactly when
//   (x_i <= x or i = 0) and (x < x_{i+1} or i = W - 2)
// which one index satisfies.  grid_sag_cell tries a candidate (the previous iterate's cell, which
// the Newton loop carries in a register), then a guess from the mean spacing, then a bisection of
// the coordinate vector: at most 2 + log2(W) dependent loads, 1 when the iterate stays in its cell.
// For a NaN coordinate the bisection ends in cell 0 and every weight is NaN.
//
// The solve (grid_sag.py:108-140): t = 0 in the local frame -- there is no base conic --
// and t += -(sag - z) / (ds/dx L + ds/dy M - N), at the point x + t L formed as the reference forms
// it.  The reference stops the whole batch when max |dt| < tol; here each ray stops when its own
// |dt| < tol, as every Newton geometry of the project does, with max_iter as the cap.  A ray whose
// iterate leaves the grid is NaN from that pass on in the reference (NaN sag -> NaN t) and is NaN
// after its final out-of-bounds test too: here its t becomes NaN and it stops.  It leaves the
// surface with NaN position and direction.
//
// Memory access.  The coordinate and node loads are per-lane table accesses.  Every index that
// comes from a floating-point value is clamped into [0, W - 2] IN floating point (a NaN becomes
// 0: grid_sag_index) before it is converted; the bisection's indices are integers between two
// such bounds; the node index is (j, i) of two such cells.  So no lane reads outside the block
// whatever its ray holds -- NaN, inf, a point far outside the grid -- and what was loaded for a
// point outside the grid is masked to NaN afterwards.  No per-ray array, no scratch, no LDS.
//
// Device coefficient block (built by ol_system_create from the public one, capi.hip); (i): an
// integer bit pattern, a scalar-unit operand:
//   [0] W (i)  [1] H (i)  [2] W - 2  [3] H - 2  [4] x_0  [5] x_{W-1}  [6] y_0  [7] y_{H-1}
//   [8] (W - 1) / (x_{W-1} - x_0)  [9] (H - 1) / (y_{H-1} - y_0)       (mean cells per millimetre)
//   then W x-coordinates, H y-coordinates, H * W sag values, row-major (row = y index)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_table.h"
#include "surface_math.h"

namespace ol {

OL_DEV float grid_sag_floor(float v) { return __builtin_floorf(v); }
OL_DEV double grid_sag_floor(double v) { return __builtin_floor(v); }
// v into [0, hi] as an index; a NaN becomes 0 (fmax / fmin return the operand that is a number)
OL_DEV int32_t grid_sag_index(float v, float hi) {
  return (int32_t)__builtin_fminf(__builtin_fmaxf(v, 0.0f), hi);
}
OL_DEV int32_t grid_sag_index(double v, double hi) {
  return (int32_t)__builtin_fmin(__builtin_fmax(v, 0.0), hi);
}

// the cell a mean spacing would give: v0 the first coordinate, inv the cells per millimetre,
// nm2 the last cell as a number
template <typename T>
OL_DEV int32_t grid_sag_guess(T x, T v0, T inv, T nm2) {
  return grid_sag_index(grid_sag_floor((x - v0) * inv), nm2);
}

// cell `k` of a vector of `n` coordinates holds x (a, b: its two ends)
template <typename T>
OL_DEV bool grid_sag_holds(T a, T b, int32_t k, int32_t n, T x) {
  return (a <= x || k == 0) && (x < b || k == n - 2);
}

// The reference's cell of x in the n coordinates v (see above) and its two ends.  cand: a cell in
// [0, n - 2] to try first.
template <typename T>
OL_DEV int32_t grid_sag_cell(const T* v, int32_t n, T x, int32_t cand, T v0, T inv, T nm2, T& a,
                             T& b) {
  a = v[cand];
  b = v[cand + 1];
  if (grid_sag_holds(a, b, cand, n, x)) return cand;
  const int32_t g = grid_sag_guess(x, v0, inv, nm2);
  a = v[g];
  b = v[g + 1];
  if (grid_sag_holds(a, b, g, n, x)) return g;
  // v[lo] <= x < v[hi], with v[0] standing for -inf and v[n - 1] for +inf; 0 < mid < n - 1
  int32_t lo = 0, hi = n - 1;
  while (hi - lo > 1) {
    const int32_t mid = (lo + hi) >> 1;
    if (v[mid] <= x) lo = mid;
    else hi = mid;
  }
  a = v[lo];
  b = v[lo + 1];
  return lo;
}

// grid_sag.py:61-101 at (x, y).  i, j: the cells to try first, and the cells found.
// c: the surface's block; blk: the same block as a GLOBAL pointer, for the per-lane loads.
template <typename T>
OL_DEV void grid_sag_eval(cptr<T> c, const T* blk, T x, T y, int32_t& i, int32_t& j, T& sag,
                          T& fx, T& fy) {
#pragma clang fp contract(off)
  using m = Math<T>;
  const int32_t W = slot_int(c), H = slot_int(c + 1);
  const T* xs = blk + kGridSagHead;
  const T* ys = xs + W;
  const T* z = ys + H;
  T x1, x2, y1, y2;
  i = grid_sag_cell<T>(xs, W, x, i, c[4], c[8], c[2], x1, x2);
  j = grid_sag_cell<T>(ys, H, y, j, c[6], c[9], c[3], y1, y2);
  const T* p = z + (j * W + i);
  const T z11 = p[0], z12 = p[1], z21 = p[W], z22 = p[W + 1];
  const T wx = x2 - x1, wy = y2 - y1;
  const T tx = m::div(x - x1, wx), ty = m::div(y - y1, wy);
  const T ux = T(1) - tx, uy = T(1) - ty;
  const T zy1 = z11 * ux + z12 * tx;
  const T zy2 = z21 * ux + z22 * tx;
  const bool inside = x >= c[4] && x <= c[5] && y >= c[6] && y <= c[7];   // (a NaN is outside)
  sag = inside ? zy1 * uy + zy2 * ty : T(__builtin_nanf(""));
  fx = m::div((z12 - z11) * uy + (z22 - z21) * ty, wx);
  fy = m::div((z21 - z11) * ux + (z22 - z12) * tx, wy);
}

// The grid-sag row of Surface._trace_real for one ray that is in the GLOBAL frame: into the
// surface's frame, the solve, the interaction (propagation, absorption, OPD, clip, Snell /
// reflection, simple coating: interact<>, unpolarised) with the normal (-ds/dx, -ds/dy, 1) / |.|
// at the hit, back to the global frame.
template <typename T, typename H>
OL_DEV Ray<T> grid_sag_step(const H& h, cptr<T> coeffs, const T* coeffs_global, Ray<T> ray) {
  using m = Math<T>;
  Ray<T> r[1] = {ray};
  into_local_frame<T, 1>(h.surf(), true, r);
  const DevSurf<T> s = h.surf();
  cptr<T> c = coeffs + s.coeff_off;
  const T* blk = coeffs_global + s.coeff_off;
  const T tol = s.cold->tol;
  const int max_iter = s.max_iter;
  const T x0 = r[0].x, y0 = r[0].y, z0 = r[0].z, L = r[0].L, M = r[0].M, N = r[0].N;
  // the cells of the starting point, by the mean spacing: the first candidates
  int32_t i = grid_sag_guess<T>(x0, c[4], c[8], c[2]);
  int32_t j = grid_sag_guess<T>(y0, c[6], c[9], c[3]);
  T t[1] = {T(0)};
  T xi = x0, yi = y0, zi = z0, sag, fx, fy;
  bool active = true;
  for (int it = 0; it < max_iter; ++it) {
    if (active) {
      grid_sag_eval<T>(c, blk, xi, yi, i, j, sag, fx, fy);
      const T f = sag - zi;                        // NaN outside the grid
      const T df = (fx * L + fy * M) - N;
      const T dt = -m::div(f, df);
      t[0] = t[0] + dt;
      active = m::abs(dt) >= tol;                  // (a NaN step stops the ray: its t is NaN)
      {
#pragma clang fp contract(off)
        xi = x0 + t[0] * L;
        yi = y0 + t[0] * M;
        zi = z0 + t[0] * N;
      }
    }
    if (!hw::wave_any(active)) break;
  }
  // the hit, the reference's final out-of-bounds test (grid_sag.py:131-140) and the normal AT the
  // hit (standard_surface.py:246-250: surface_normal interpolates once more): one evaluation
  grid_sag_eval<T>(c, blk, xi, yi, i, j, sag, fx, fy);
  const T poison = sag * T(0);                     // 0, or NaN for a ray outside the grid
  t[0] = t[0] + poison;
  r[0].x = xi + poison;
  r[0].y = yi + poison;
  r[0].z = zi + poison;
  const T im = m::rsqrt(m::fma(fx, fx, m::fma(fy, fy, T(1)))) + poison;
  const T nx[1] = {-fx * im}, ny[1] = {-fy * im}, nz[1] = {im};
  Prt<T, 0> P[1];
  bool prt_fresh = false;
  interact<T, 1, 0, true>(s, h.optics(), coeffs, t, nx, ny, nz, r, P, prt_fresh);
  return to_global<T>(s, r[0]);
}

}  // namespace ol
