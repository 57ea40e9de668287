// main.hip -- TEST INFRASTRUCTURE: the grid-sag step of optiland_amd/csrc/grid_sag_device.h,
// compiled for the host (OL_HOST_MATH) and run ray by ray as a stand-alone program.
//
//   hostgrid step <case file>     grid_sag_trace_kernel's body for every ray: one line per ray
//   hostgrid cells <case file>    grid_sag_cell for every probe coordinate on both axes of the
//                                   case's grid, from the candidates 0, the last cell and the
//                                   mean-spacing guess: one line per coordinate; exit 1 when the
//                                   candidates disagree
//   hostgrid refuse <case file>   every range-walking entry point on the case's system: one
//                                   line per call with its return code (no launch happens)
//   hostgrid create <case file>   ol_system_create alone: its return code and message
//   hostgrid rules <case file>    the argument rules of ol_trace_grid_sag (single_host.h) on
//                                   the case's system: one line per call
//
// Linked with the host-only compile of csrc/capi.hip (ol_system_create builds the table the
// kernel reads) and tests/hostmath/harness.hip (the stand-in for the few HIP runtime calls
// capi.hip makes) -- the objects tests/hostmath/build.py leaves behind, plain or with
// AddressSanitizer + UndefinedBehaviorSanitizer: the coefficient buffers are heap blocks of exactly
// the table's size, so a load outside the block is reported.  A program of its own: nothing is
// loaded into an interpreter.  Not a fallback: nothing under optiland_amd/ knows about it.
//
// Case file (little endian): 8 int64 -- magic, n_surf, n_wl, n_coeff, n, surface, n_probe, dtype
// (0 = fp32, 1 = fp64); then n_surf ol_surface_desc, n_surf x n_wl ol_surface_optics, n_coeff
// doubles, 8 planes of n doubles (x, y, z, L, M, N, i, opd), n_probe doubles.  The loader,
// `step`'s loop, `refuse`, the rules and `main`: tests/hostsingle/host_common.h.
#define OL_HOST_MATH 1
#include "../../optiland_amd/csrc/grid_sag_device.h"
#include "../hostsingle/host_common.h"

namespace {

using host::Case;

// (the case names no wavelength: index 0 throughout)
constexpr host::Program kProgram{"hostgrid", "step|cells|refuse|create|rules",
                                 0x444952476c6fLL /* "olGRID" */, ol::kSingleGridSag,
                                 false, true, "not a grid-sag row"};

bool grid_row(const Case& c, const ol::SystemView& v) {
  const int64_t s = c.h[5];
  if (s >= 0 && s < v.n_surf && ol::is_grid_sag_kind(v.geom[s])) return true;
  printf("error: surface %lld is not a grid-sag row of the case\n", (long long)s);
  return false;
}

// grid_sag_trace_kernel (grid_sag.hip) for every ray
template <typename T>
int step(const Case& c, const ol::SystemView& v) {
  using namespace ol;
  if (!grid_row(c, v)) return 1;
  return host::run_step<T>(
      c, v, 0,
      [](const SingleArgs<T>& a, const Ray<T>& r) {
        return grid_sag_step<T>(single_fetched(a), as_const(a.coeffs), a.coeffs, r);
      },
      [](const Ray<T>& g) { return g.L != g.L; });
}

// the cell of every probe coordinate on either axis, whatever candidate the search starts from
template <typename T>
int cells(const Case& c, const ol::SystemView& v) {
  using namespace ol;
  if (!grid_row(c, v)) return 1;
  const Rows<T> t = rows_of<T>(v);
  const T* blk = t.coeffs + t.hot[c.h[5]].coeff_off;
  const int32_t W = slot_int(as_const(blk)), H = slot_int(as_const(blk + 1));
  const T* xs = blk + kGridSagHead;
  const T* ys = xs + W;
  int bad = 0;
  for (double p : c.probe) {
    const T x = (T)p;
    int32_t got[2];
    for (int ax = 0; ax < 2; ++ax) {
      const T* vv = ax ? ys : xs;
      const int32_t n = ax ? H : W;
      const T v0 = blk[ax ? 6 : 4], inv = blk[ax ? 9 : 8], nm2 = blk[ax ? 3 : 2];
      const int32_t cand[3] = {0, n - 2, grid_sag_guess<T>(x, v0, inv, nm2)};
      T a, b;
      got[ax] = grid_sag_cell<T>(vv, n, x, cand[0], v0, inv, nm2, a, b);
      for (int k = 1; k < 3; ++k)
        if (grid_sag_cell<T>(vv, n, x, cand[k], v0, inv, nm2, a, b) != got[ax]) bad = 1;
      if (a != vv[got[ax]] || b != vv[got[ax] + 1]) bad = 1;
    }
    printf("cell %.17g %d %d\n", (double)x, got[0], got[1]);
  }
  return bad;
}

}  // namespace

int main(int argc, char** argv) {
  return host::main_of(kProgram, argc, argv,
                       [](const char* mode, Case& c, ol_system* sys, const ol::SystemView& v) {
    if (strcmp(mode, "step") == 0) return c.h[7] ? step<double>(c, v) : step<float>(c, v);
    if (strcmp(mode, "cells") == 0) return c.h[7] ? cells<double>(c, v) : cells<float>(c, v);
    if (strcmp(mode, "refuse") == 0) return host::refuse(c, sys, 0, false);
    host::rules(kProgram, c, sys, 0);
    return 0;
  });
}
