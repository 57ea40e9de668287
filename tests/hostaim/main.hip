// main.hip -- TEST INFRASTRUCTURE: the ray-aiming solve of optiland_amd/csrc/ray_aim_device.h,
// compiled for the host (OL_HOST_MATH) and run ray by ray as a stand-alone program.
//
//   hostaim solve <case file>      the solution of one case, one line per ray
//   hostaim validate <case file>   the argument rules of ol_aim_rays (ray_aim_host.h) on the
//                                  case's system: one line per broken call
//
// Linked with the host-only compile of csrc/capi.hip (ol_system_create builds the table the
// kernels read) and tests/hostmath/harness.hip (the stand-in for the few HIP runtime calls
// capi.hip makes) -- the objects tests/hostmath/build.py leaves behind, plain or with
// AddressSanitizer + UndefinedBehaviorSanitizer.  A program of its own: nothing is loaded into
// an interpreter.  Not a fallback: nothing under optiland_amd/ knows about it.
//
// Case file (little endian): 12 int64 -- magic, n_surf, n_wl, n_coeff, n, first, stop,
// wavelength index, max_iter, infinite, use_guess, raygen flags; 3 doubles -- r_stop, jacobian,
// tol; 11 doubles -- the generator's scalars in the order of ol_raygen_params (the three
// integers as doubles); 4 doubles -- hx0, hy0, vx0, vy0; then n_surf ol_surface_desc,
// n_surf x n_wl ol_surface_optics, n_coeff doubles; then px[n], py[n] and, with use_guess,
// six planes of n doubles.
#define OL_HOST_MATH 1
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/optiland_hip.h"
#include "../../optiland_amd/csrc/ray_aim_device.h"
#include "../../optiland_amd/csrc/ray_aim_host.h"
#include "../../optiland_amd/csrc/raygen_device.h"
#include "../../optiland_amd/csrc/system_view.h"
#include "../../optiland_amd/csrc/trace_launch.h"

namespace {

constexpr int64_t kMagic = 0x4d49416c6fLL;   // "olAIM"

struct Case {
  int64_t h[12];
  double scal[3], rg[11], uni[4];
  std::vector<ol_surface_desc> surf;
  std::vector<ol_surface_optics> optics;
  std::vector<double> coeffs, px, py, guess[6];
};

bool read_exact(FILE* f, void* dst, size_t bytes) { return bytes == 0 || fread(dst, bytes, 1, f) == 1; }

bool load(const char* path, Case& c) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  bool ok = read_exact(f, c.h, sizeof c.h) && c.h[0] == kMagic;
  ok = ok && read_exact(f, c.scal, sizeof c.scal) && read_exact(f, c.rg, sizeof c.rg) &&
       read_exact(f, c.uni, sizeof c.uni);
  // sizes a case file of this suite stays far inside: a corrupt header must not allocate
  ok = ok && c.h[1] > 0 && c.h[1] < 4096 && c.h[2] > 0 && c.h[2] < 64 && c.h[3] >= 0 &&
       c.h[3] < (1 << 24) && c.h[4] >= 0 && c.h[4] < (1 << 24);
  if (ok) {
    const size_t ns = (size_t)c.h[1], nw = (size_t)c.h[2], nc = (size_t)c.h[3], n = (size_t)c.h[4];
    c.surf.resize(ns);
    c.optics.resize(ns * nw);
    c.coeffs.resize(nc);
    c.px.resize(n);
    c.py.resize(n);
    ok = read_exact(f, c.surf.data(), ns * sizeof(ol_surface_desc)) &&
         read_exact(f, c.optics.data(), ns * nw * sizeof(ol_surface_optics)) &&
         read_exact(f, c.coeffs.data(), nc * sizeof(double)) &&
         read_exact(f, c.px.data(), n * sizeof(double)) &&
         read_exact(f, c.py.data(), n * sizeof(double));
    if (ok && c.h[10])
      for (auto& g : c.guess) {
        g.resize(n);
        ok = ok && read_exact(f, g.data(), n * sizeof(double));
      }
  }
  fclose(f);
  return ok;
}

ol_aim_params params_of(const Case& c) {
  ol_aim_params p{};
  p.stop_radius = c.scal[0];
  p.jacobian = c.scal[1];
  p.tol = c.scal[2];
  p.max_iter = (int32_t)c.h[8];
  p.infinite = (int32_t)c.h[9];
  ol_raygen_params& g = p.raygen;
  g.object_infinite = (int32_t)c.rg[0];
  g.field_kind = (int32_t)c.rg[1];
  g.EPL = c.rg[2]; g.EPD = c.rg[3]; g.max_field = c.rg[4]; g.offset = c.rg[5];
  g.z_first = c.rg[6]; g.tele_dz = c.rg[7]; g.apod_a = c.rg[8]; g.apod_b = c.rg[9];
  g.apod_kind = (int32_t)c.rg[10];
  return p;
}

// aim_rays_kernel (ray_aim.hip) for ray i, statement by statement: a "wave" of one ray
template <int NR>
uint32_t solve_one(const ol::AimTable& t, const ol::AimConsts& k, const Case& c,
                   const ol::RaygenIn<double>& in, const ol::RaygenConsts<double>& rgc, int64_t i,
                   double (&o)[6], int32_t& updates) {
  using namespace ol;
  uint32_t status = 0;
  double px = c.px[i], py = c.py[i];
  if (c.h[10]) {
    for (int q = 0; q < 6; ++q) o[q] = c.guess[q][i];
  } else {
    double vx = in.vx0, vy = in.vy0;
    raygen_pupil<double>(in.flags, vx, vy, px, py, status);
    raygen_one<double>(rgc, in.tx0, in.ty0, px, py, vx, vy, o);
  }
  status |= aim_one<NR>(t, k, px, py, o, updates, status);
  return status;
}

int solve(const Case& c, ol_system* sys) {
  using namespace ol;
  const ol_aim_params p = params_of(c);
  static const double none = 0.0;   // (an empty case still hands over two planes)
  ol_raygen_inputs in{};
  in.px = c.px.empty() ? &none : c.px.data();
  in.py = c.py.empty() ? &none : c.py.data();
  in.hx0 = c.uni[0]; in.hy0 = c.uni[1]; in.vx0 = c.uni[2]; in.vy0 = c.uni[3];
  in.flags = (uint32_t)c.h[11];
  const void* gp[6];
  for (int q = 0; q < 6; ++q) gp[q] = c.guess[q].empty() ? &none : c.guess[q].data();
  std::vector<double> out[6];
  void* op[6];
  for (int q = 0; q < 6; ++q) {
    out[q].assign((size_t)c.h[4] + 1, 0.0);
    op[q] = out[q].data();
  }
  uint32_t status = 0;
  if (int rc = aim_check(sys, c.h[4], (int32_t)c.h[7], (int32_t)c.h[5], (int32_t)c.h[6], &p, &in,
                         c.h[10] ? gp : nullptr, op, &status)) {
    printf("error %d %s\n", rc, ol_last_error());
    return 1;
  }
  const SystemView v = system_view(sys);
  const AimTable t{v.surf, v.cold, v.optics, v.coeffs, (int32_t)c.h[5], (int32_t)c.h[6], v.n_wl,
                   (int32_t)c.h[7]};
  const AimConsts k{p.stop_radius, p.jacobian, p.tol, p.max_iter, p.infinite != 0};
  const ol_raygen_params& g = p.raygen;
  const RaygenDev rg{g.object_infinite, g.field_kind, g.EPL,    g.EPD,    g.max_field, g.offset,
                     g.z_first,         g.tele_dz,    g.apod_a, g.apod_b, g.apod_kind};
  RaygenIn<double> ri{};
  ri.hx0 = in.hx0; ri.hy0 = in.hy0; ri.vx0 = in.vx0; ri.vy0 = in.vy0;
  ri.flags = in.flags;
  uniform_field_tangents<double>(rg, ri);
  const RaygenConsts<double> rgc(rg);
  const bool lean = system_newton_family(sys, t.first, t.stop) == kNrNone;
  for (int64_t i = 0; i < c.h[4]; ++i) {
    double o[6];
    int32_t updates = 0;
    const uint32_t bits = lean ? solve_one<kNrNone>(t, k, c, ri, rgc, i, o, updates)
                               : solve_one<kNrGeneric>(t, k, c, ri, rgc, i, o, updates);
    status |= bits;
    printf("ray %lld %.17g %.17g %.17g %.17g %.17g %.17g %d %u\n", (long long)i, o[0], o[1], o[2],
           o[3], o[4], o[5], updates, bits);
  }
  printf("status %u\n", status);
  return 0;
}

int validate(const Case& c, ol_system* sys) {
  using namespace ol;
  const ol_aim_params good = params_of(c);
  double plane = 0.0;
  ol_raygen_inputs in{};
  in.px = &plane;
  in.py = &plane;
  void* op[6] = {&plane, &plane, &plane, &plane, &plane, &plane};
  const void* gp[6] = {&plane, &plane, &plane, &plane, &plane, &plane};
  uint32_t status = 0;
  const int32_t wl = (int32_t)c.h[7], first = (int32_t)c.h[5], stop = (int32_t)c.h[6];
  const int32_t n_surf = (int32_t)c.h[1];
  auto say = [](const char* what, int rc) { printf("%s: %d %s\n", what, rc, rc ? ol_last_error() : "ok"); };
  say("good", aim_check(sys, 1, wl, first, stop, &good, &in, nullptr, op, &status));
  say("good guess", aim_check(sys, 1, wl, first, stop, &good, &in, gp, op, &status));
  say("empty", aim_check(sys, 0, wl, first, stop, &good, &in, nullptr, op, &status));
  say("null system", aim_check(nullptr, 1, wl, first, stop, &good, &in, nullptr, op, &status));
  say("null params", aim_check(sys, 1, wl, first, stop, nullptr, &in, nullptr, op, &status));
  say("null inputs", aim_check(sys, 1, wl, first, stop, &good, nullptr, nullptr, op, &status));
  { ol_raygen_inputs b = in; b.py = nullptr;
    say("null py", aim_check(sys, 1, wl, first, stop, &good, &b, nullptr, op, &status)); }
  { ol_raygen_inputs b = in; b.hx = &plane;
    say("hx without hy", aim_check(sys, 1, wl, first, stop, &good, &b, nullptr, op, &status)); }
  say("null status", aim_check(sys, 1, wl, first, stop, &good, &in, nullptr, op, nullptr));
  say("null out", aim_check(sys, 1, wl, first, stop, &good, &in, nullptr, nullptr, &status));
  { void* b[6] = {&plane, &plane, &plane, nullptr, &plane, &plane};
    say("null out plane", aim_check(sys, 1, wl, first, stop, &good, &in, nullptr, b, &status)); }
  { const void* b[6] = {&plane, nullptr, &plane, &plane, &plane, &plane};
    say("null guess plane", aim_check(sys, 1, wl, first, stop, &good, &in, b, op, &status)); }
  say("negative count", aim_check(sys, -1, wl, first, stop, &good, &in, nullptr, op, &status));
  say("wavelength", aim_check(sys, 1, (int32_t)c.h[2], first, stop, &good, &in, nullptr, op, &status));
  say("stop past the table", aim_check(sys, 1, wl, first, n_surf, &good, &in, nullptr, op, &status));
  say("negative first", aim_check(sys, 1, wl, -1, stop, &good, &in, nullptr, op, &status));
  say("first past stop", aim_check(sys, 1, wl, stop + 1, stop, &good, &in, nullptr, op, &status));
  const double nan = std::nan(""), inf = INFINITY;
  { ol_aim_params b = good; b.max_iter = -1;
    say("max_iter -1", aim_check(sys, 1, wl, first, stop, &b, &in, nullptr, op, &status)); }
  { ol_aim_params b = good; b.max_iter = OL_AIM_MAX_ITER + 1;
    say("max_iter 1001", aim_check(sys, 1, wl, first, stop, &b, &in, nullptr, op, &status)); }
  { ol_aim_params b = good; b.max_iter = 0;
    say("max_iter 0", aim_check(sys, 1, wl, first, stop, &b, &in, nullptr, op, &status)); }
  { ol_aim_params b = good; b.tol = -1e-9;
    say("tol negative", aim_check(sys, 1, wl, first, stop, &b, &in, nullptr, op, &status)); }
  { ol_aim_params b = good; b.tol = nan;
    say("tol nan", aim_check(sys, 1, wl, first, stop, &b, &in, nullptr, op, &status)); }
  { ol_aim_params b = good; b.tol = inf;
    say("tol inf", aim_check(sys, 1, wl, first, stop, &b, &in, nullptr, op, &status)); }
  { ol_aim_params b = good; b.stop_radius = nan;
    say("r_stop nan", aim_check(sys, 1, wl, first, stop, &b, &in, nullptr, op, &status)); }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3 || (strcmp(argv[1], "solve") != 0 && strcmp(argv[1], "validate") != 0)) {
    fprintf(stderr, "usage: hostaim solve|validate <case file>\n");
    return 2;
  }
  Case c;
  if (!load(argv[2], c)) {
    fprintf(stderr, "hostaim: cannot read the case file %s\n", argv[2]);
    return 2;
  }
  ol_system* sys = nullptr;
  if (ol_system_create(c.surf.data(), (int32_t)c.surf.size(), c.coeffs.empty() ? nullptr : c.coeffs.data(),
                       (int32_t)c.coeffs.size(), c.optics.data(), (int32_t)c.h[2], &sys) != OL_OK) {
    fprintf(stderr, "hostaim: ol_system_create: %s\n", ol_last_error());
    return 2;
  }
  const int rc = strcmp(argv[1], "solve") == 0 ? solve(c, sys) : validate(c, sys);
  ol_system_destroy(sys);
  return rc;
}
