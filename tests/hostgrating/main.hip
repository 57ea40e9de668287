// main.hip -- TEST INFRASTRUCTURE: the grating step of optiland_amd/csrc/grating_device.h,
// compiled for the host (OL_HOST_MATH) and run ray by ray as a stand-alone program.
//
//   hostgrating step <case file>     grating_trace_kernel's body for every ray: one line per ray
//   hostgrating refuse <case file>   every range-walking entry point on the case's system: one
//                                    line per call with its return code (no launch happens)
//   hostgrating create <case file>   ol_system_create alone: its return code and message
//   hostgrating rules <case file>    the argument rules of ol_trace_grating (single_host.h) on
//                                    the case's system: one line per call
//
// Linked with the host-only compile of csrc/capi.hip (ol_system_create builds the table the
// kernel reads) and tests/hostmath/harness.hip (the stand-in for the few HIP runtime calls
// capi.hip makes) -- the objects tests/hostmath/build.py leaves behind, plain or with
// AddressSanitizer + UndefinedBehaviorSanitizer.  A program of its own: nothing is loaded into
// an interpreter.  Not a fallback: nothing under optiland_amd/ knows about it.
//
// Case file (little endian), the layout of tests/hostforbes with the wavelength behind the
// header: 8 int64 -- magic, n_surf, n_wl, n_coeff, n, surface, wavelength index, dtype (0 = fp32,
// 1 = fp64); one double -- the wavelength in micrometres; then n_surf ol_surface_desc,
// n_surf x n_wl ol_surface_optics, n_coeff doubles, 8 planes of n doubles (x, y, z, L, M, N, i,
// opd).  The loader, `step`'s loop, `refuse`, the shared rules and `main`:
// tests/hostsingle/host_common.h.
#define OL_HOST_MATH 1
#include "../../optiland_amd/csrc/grating_device.h"
#include "../hostsingle/host_common.h"

namespace {

using host::Case;
using host::say;

constexpr host::Program kProgram{"hostgrating", "step|refuse|create|rules",
                                 0x544152476c6fLL /* "olGRAT" */, ol::kSingleGrating,
                                 true, false, "not a grating row"};

// grating_trace_kernel (grating.hip) for every ray
template <typename T>
int step(const Case& c, const ol::SystemView& v) {
  using namespace ol;
  const int64_t s = c.h[5];
  if (s < 0 || s >= v.n_surf || !is_grating_kind(v.geom[s]) || c.h[6] < 0 || c.h[6] >= v.n_wl) {
    printf("error: surface %lld is not a grating row of the case / bad wavelength index\n",
           (long long)s);
    return 1;
  }
  const T wavelength = (T)c.wavelength;
  return host::run_step<T>(
      c, v, (int32_t)c.h[6],
      [wavelength](const SingleArgs<T>& a, const Ray<T>& r) {
        return grating_step<T>(single_fetched(a), as_const(a.coeffs), r, wavelength);
      },
      [](const Ray<T>& g) { return g.L != g.L && g.x == g.x; });
}

// ol_trace_grating's own rules, then the precedence: the first broken rule answers
int rules(Case& c, ol_system* sys) {
  const int32_t wl = (int32_t)c.h[6], s = (int32_t)c.h[5], n_surf = (int32_t)c.h[1];
  const int64_t n = c.h[4];
  const double w = c.wavelength;
  const auto check = host::rules(kProgram, c, sys, wl);
  say("all at once", check(sys, (ol_dtype)5, -1, nullptr, -1, 0.0, nullptr, 0, n_surf, ~0u));
  say("all but dtype", check(sys, OL_F64, -1, nullptr, -1, 0.0, nullptr, 0, n_surf, ~0u));
  say("surface before wavelength", check(sys, OL_F64, n, nullptr, -1, 0.0, nullptr, 0, n_surf, ~0u));
  say("wavelength index before wavelength_um", check(sys, OL_F64, n, nullptr, -1, 0.0, nullptr, 0, s, ~0u));
  say("wavelength_um before flags", check(sys, OL_F64, n, nullptr, wl, 0.0, nullptr, 0, s, ~0u));
  say("flags before planes", check(sys, OL_F64, n, nullptr, wl, w, nullptr, 0, s, ~0u));
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  return host::main_of(kProgram, argc, argv,
                       [](const char* mode, Case& c, ol_system* sys, const ol::SystemView& v) {
    if (strcmp(mode, "step") == 0) return c.h[7] ? step<double>(c, v) : step<float>(c, v);
    if (strcmp(mode, "refuse") == 0) return host::refuse(c, sys, (int32_t)c.h[6], true);
    return rules(c, sys);
  });
}
