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
//   hostgrid rules <case file>    the argument rules of ol_trace_grid_sag (grid_sag_host.h) on
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
// doubles, 8 planes of n doubles (x, y, z, L, M, N, i, opd), n_probe doubles.
#define OL_HOST_MATH 1
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/optiland_hip.h"
#include "../../optiland_amd/csrc/grid_sag_device.h"
#include "../../optiland_amd/csrc/grid_sag_host.h"
#include "../../optiland_amd/csrc/ray_aim_host.h"
#include "../../optiland_amd/csrc/system_view.h"

namespace {

constexpr int64_t kMagic = 0x444952476c6fLL;   // "olGRID"

struct Case {
  int64_t h[8];
  std::vector<ol_surface_desc> surf;
  std::vector<ol_surface_optics> optics;
  std::vector<double> coeffs, plane[8], probe;
};

bool read_exact(FILE* f, void* dst, size_t bytes) { return bytes == 0 || fread(dst, bytes, 1, f) == 1; }

bool load(const char* path, Case& c) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  bool ok = read_exact(f, c.h, sizeof c.h) && c.h[0] == kMagic;
  // sizes a case file of this suite stays far inside: a corrupt header must not allocate
  ok = ok && c.h[1] > 0 && c.h[1] < 4096 && c.h[2] > 0 && c.h[2] < 64 && c.h[3] >= 0 &&
       c.h[3] < (1 << 24) && c.h[4] >= 0 && c.h[4] < (1 << 24) && c.h[6] >= 0 && c.h[6] < (1 << 24);
  if (ok) {
    const size_t ns = (size_t)c.h[1], nw = (size_t)c.h[2], nc = (size_t)c.h[3], n = (size_t)c.h[4];
    c.surf.resize(ns);
    c.optics.resize(ns * nw);
    c.coeffs.resize(nc);
    ok = read_exact(f, c.surf.data(), ns * sizeof(ol_surface_desc)) &&
         read_exact(f, c.optics.data(), ns * nw * sizeof(ol_surface_optics)) &&
         read_exact(f, c.coeffs.data(), nc * sizeof(double));
    for (auto& p : c.plane) {
      p.resize(n);
      ok = ok && read_exact(f, p.data(), n * sizeof(double));
    }
    c.probe.resize((size_t)c.h[6]);
    ok = ok && read_exact(f, c.probe.data(), c.probe.size() * sizeof(double));
  }
  fclose(f);
  return ok;
}

template <typename T>
struct Rows {
  const ol::DevSurfHot<T>* hot;
  const ol::DevSurfCold<T>* cold;
  const ol::DevOptics<T>* opt;
  const T* coeffs;
};
template <typename T>
Rows<T> rows_of(const ol::SystemView& v);
template <>
Rows<double> rows_of<double>(const ol::SystemView& v) { return {v.surf, v.cold, v.optics, v.coeffs}; }
template <>
Rows<float> rows_of<float>(const ol::SystemView& v) {
  return {v.surf32, v.cold32, v.optics32, v.coeffs32};
}

bool grid_row(const Case& c, const ol::SystemView& v) {
  const int64_t s = c.h[5];
  if (s >= 0 && s < v.n_surf && ol::is_grid_sag_kind(v.geom[s])) return true;
  printf("error: surface %lld is not a grid-sag row of the case\n", (long long)s);
  return false;
}

// grid_sag_trace_kernel (grid_sag.hip) for ray i, statement by statement
template <typename T>
int step(const Case& c, const ol::SystemView& v) {
  using namespace ol;
  if (!grid_row(c, v)) return 1;
  const int64_t s = c.h[5];
  const Rows<T> t = rows_of<T>(v);
  const SurfFetched<T> h{as_const(t.hot + s), as_const(t.cold + s), as_const(t.opt + s * v.n_wl)};
  for (int64_t i = 0; i < c.h[4]; ++i) {
    Ray<T> r;
    r.x = (T)c.plane[0][i]; r.y = (T)c.plane[1][i]; r.z = (T)c.plane[2][i];
    r.L = (T)c.plane[3][i]; r.M = (T)c.plane[4][i]; r.N = (T)c.plane[5][i];
    r.i = (T)c.plane[6][i]; r.opd = (T)c.plane[7][i];
    const Ray<T> g = grid_sag_step<T>(h, as_const(t.coeffs), t.coeffs, r);
    const uint32_t bits = (g.L != g.L) ? OL_STATUS_NAN_DIRECTION : 0u;
    printf("ray %lld %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %u\n", (long long)i,
           (double)g.x, (double)g.y, (double)g.z, (double)g.L, (double)g.M, (double)g.N,
           (double)g.i, (double)g.opd, bits);
  }
  return 0;
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

// every entry point that walks a surface range, on a range that holds the case's grid-sag row:
// OL_EUNSUPPORTED before anything is launched (the arguments behind the range are never read)
int refuse(const Case& c, ol_system* sys) {
  const int32_t last = (int32_t)c.h[1] - 1, wl = 0, s = (int32_t)c.h[5];
  double plane[4] = {0, 0, 0, 0};
  void* rays[8] = {plane, plane, plane, plane, plane, plane, plane, plane};
  uint32_t status = 0;
  int32_t iters[8192] = {0};
  ol_raygen_params rg{};
  ol_raygen_inputs in{};
  in.px = plane;
  in.py = plane;
  auto say = [](const char* what, int rc) {
    printf("%s: %d %s\n", what, rc, rc ? ol_last_error() : "ok");
  };
  say("ol_trace", ol_trace(sys, OL_F64, 1, rays, wl, nullptr, 0, nullptr, 0, last,
                           OL_TRACE_WRITE_RAYS, &status, nullptr));
  say("ol_trace one surface", ol_trace(sys, OL_F32, 1, rays, wl, nullptr, 0, nullptr, s, s,
                                       OL_TRACE_WRITE_RAYS, &status, nullptr));
  say("ol_trace_ex", ol_trace_ex(sys, OL_F64, 1, rays, wl, nullptr, 0, nullptr, 0, last,
                                 OL_TRACE_WRITE_RAYS, &status, nullptr, nullptr));
  say("ol_newton_count", ol_newton_count(sys, OL_F64, 1, rays, wl, 0, last, iters, 0, nullptr));
  say("ol_trace_generate", ol_trace_generate(sys, OL_F64, 1, &rg, &in, wl, plane, 1, nullptr,
                                             nullptr, 0, &status, nullptr, nullptr));
  void* hits[3] = {plane, plane, plane};
  double out8[8] = {0};
  say("ol_trace_spot", ol_trace_spot(sys, OL_F64, 1, &rg, &in, 0.0, 0.0, wl, hits, out8, &status,
                                     nullptr));
  ol_spot_cell cell{};
  cell.wavelength_index = wl;
  say("ol_trace_spot_batch", ol_trace_spot_batch(sys, OL_F64, 1, &rg, &in, 1, &cell, nullptr, 0,
                                                 out8, &status, nullptr));
  ol_wavefront_params wp{};
  double mom[OL_WAVEFRONT_REFERENCE_DOUBLES + 16] = {0};
  void* opd_out[3] = {plane, plane, plane};
  say("ol_trace_opd", ol_trace_opd(sys, OL_F64, 1, &rg, &in, &wp, wl, plane, plane, opd_out, mom,
                                   &status, nullptr));
  say("ol_wavefront_reference", ol_wavefront_reference(sys, OL_F64, &rg, &in, &wp, 0.0, 0, wl, mom,
                                                       mom, &status, nullptr));
  say("ol_trace_opd_dev", ol_trace_opd_dev(sys, OL_F64, 1, &rg, &in, mom, wl, plane, plane,
                                           opd_out, mom, &status, nullptr));
  ol_aim_params ap{};
  ap.max_iter = 1;
  void* aim_out[6] = {plane, plane, plane, plane, plane, plane};
  say("ol_aim_rays", ol::aim_check(sys, 1, wl, 0, last, &ap, &in, nullptr, aim_out, &status));
  return 0;
}

// ol_trace_grid_sag's own rules, one broken at a time (every plane is a real one of the case)
int rules(Case& c, ol_system* sys) {
  using namespace ol;
  const int32_t wl = 0, s = (int32_t)c.h[5], n_surf = (int32_t)c.h[1];
  const int64_t n = c.h[4];
  std::vector<double> row(8 * (size_t)n + 1);
  void* rays[8];
  for (int k = 0; k < 8; ++k) rays[k] = c.plane[k].data();
  auto say = [](const char* what, int rc) {
    printf("%s: %d %s\n", what, rc, rc ? ol_last_error() : "ok");
  };
  const uint32_t wr = OL_TRACE_WRITE_RAYS;
  say("good", grid_sag_check(sys, OL_F64, n, rays, wl, row.data(), n, s, 0));
  say("good fp32 midrange", grid_sag_check(sys, OL_F32, n, rays, wl, nullptr, 0, s,
                                           wr | OL_TRACE_MIDRANGE));
  say("empty", grid_sag_check(sys, OL_F64, 0, nullptr, wl, nullptr, 0, s, 0));
  say("null system", grid_sag_check(nullptr, OL_F64, n, rays, wl, row.data(), n, s, 0));
  say("dtype", grid_sag_check(sys, (ol_dtype)5, n, rays, wl, row.data(), n, s, 0));
  say("negative count", grid_sag_check(sys, OL_F64, -1, rays, wl, row.data(), n, s, 0));
  say("surface -1", grid_sag_check(sys, OL_F64, n, rays, wl, row.data(), n, -1, 0));
  say("surface past the table", grid_sag_check(sys, OL_F64, n, rays, wl, row.data(), n, n_surf, 0));
  say("not a grid-sag row", grid_sag_check(sys, OL_F64, n, rays, wl, row.data(), n, s + 1, 0));
  say("wavelength", grid_sag_check(sys, OL_F64, n, rays, (int32_t)c.h[2], row.data(), n, s, 0));
  say("wavelength -1", grid_sag_check(sys, OL_F64, n, rays, -1, row.data(), n, s, 0));
  say("flags", grid_sag_check(sys, OL_F64, n, rays, wl, row.data(), n, s, OL_TRACE_PRT_COMPLEX));
  say("too many", grid_sag_check(sys, OL_F64, ((int64_t)0x7fffffff * 64) + 1, rays, wl, nullptr, 0,
                                 s, wr));
  say("null rays", grid_sag_check(sys, OL_F64, n, nullptr, wl, row.data(), n, s, 0));
  { void* b[8];
    for (int k = 0; k < 8; ++k) b[k] = k == 5 ? nullptr : rays[k];
    say("null plane", grid_sag_check(sys, OL_F64, n, b, wl, row.data(), n, s, 0)); }
  say("stride", grid_sag_check(sys, OL_F64, n, rays, wl, row.data(), n - 1, s, 0));
  say("nothing to write", grid_sag_check(sys, OL_F64, n, rays, wl, nullptr, 0, s, 0));
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const char* modes[] = {"step", "refuse", "create", "rules", "cells"};
  int mode = -1;
  for (int k = 0; k < 5 && argc == 3; ++k)
    if (strcmp(argv[1], modes[k]) == 0) mode = k;
  if (mode < 0) {
    fprintf(stderr, "usage: hostgrid step|cells|refuse|create|rules <case file>\n");
    return 2;
  }
  Case c;
  if (!load(argv[2], c)) {
    fprintf(stderr, "hostgrid: cannot read the case file %s\n", argv[2]);
    return 2;
  }
  ol_system* sys = nullptr;
  const int rc = ol_system_create(c.surf.data(), (int32_t)c.surf.size(),
                                  c.coeffs.empty() ? nullptr : c.coeffs.data(),
                                  (int32_t)c.coeffs.size(), c.optics.data(), (int32_t)c.h[2], &sys);
  if (mode == 2) {
    printf("create: %d %s\n", rc, rc ? ol_last_error() : "ok");
    ol_system_destroy(sys);
    return 0;
  }
  if (rc != OL_OK) {
    fprintf(stderr, "hostgrid: ol_system_create: %s\n", ol_last_error());
    return 2;
  }
  const ol::SystemView v = ol::system_view(sys);
  int out = 0;
  if (mode == 0) out = c.h[7] ? step<double>(c, v) : step<float>(c, v);
  if (mode == 1) out = refuse(c, sys);
  if (mode == 3) out = rules(c, sys);
  if (mode == 4) out = c.h[7] ? cells<double>(c, v) : cells<float>(c, v);
  ol_system_destroy(sys);
  return out;
}
