// main.hip -- TEST INFRASTRUCTURE: the Forbes surface step of optiland_amd/csrc/forbes_device.h,
// compiled for the host (OL_HOST_MATH) and run ray by ray as a stand-alone program.
//
//   hostforbes step <case file>     forbes_trace_kernel's body for every ray: one line per ray
//   hostforbes grid <case file>     sag and unit normal at the points (planes 0 and 1)
//   hostforbes refuse <case file>   every range-walking entry point on the case's system: one
//                                   line per call with its return code (no launch happens)
//   hostforbes create <case file>   ol_system_create alone: its return code and message
//   hostforbes rules <case file>    the argument rules of ol_trace_forbes (single_host.h) on the
//                                   case's system: one line per call
//
// Linked with the host-only compile of csrc/capi.hip (ol_system_create builds the table the
// kernel reads) and tests/hostmath/harness.hip (the stand-in for the few HIP runtime calls
// capi.hip makes) -- the objects tests/hostmath/build.py leaves behind, plain or with
// AddressSanitizer + UndefinedBehaviorSanitizer.  A program of its own: nothing is loaded into
// an interpreter.  Not a fallback: nothing under optiland_amd/ knows about it.
//
// Case file (little endian): 8 int64 -- magic, n_surf, n_wl, n_coeff, n, surface, wavelength
// index, dtype (0 = fp32, 1 = fp64); then n_surf ol_surface_desc, n_surf x n_wl
// ol_surface_optics, n_coeff doubles, 8 planes of n doubles (x, y, z, L, M, N, i, opd).
// The loader, `step`'s loop, `refuse`, the shared rules and `main`: tests/hostsingle/host_common.h.
#define OL_HOST_MATH 1
#include "../../optiland_amd/csrc/forbes_device.h"
#include "../hostsingle/host_common.h"

namespace {

using host::Case;
using host::say;

constexpr host::Program kProgram{"hostforbes", "step|grid|refuse|create|rules",
                                 0x534252466c6fLL /* "olFRBS" */, ol::kSingleForbes,
                                 false, false, "not a forbes row"};

bool forbes_row(const Case& c, const ol::SystemView& v) {
  const int64_t s = c.h[5];
  if (s < 0 || s >= v.n_surf || !ol::is_forbes_kind(v.geom[s]) || c.h[6] < 0 || c.h[6] >= v.n_wl) {
    printf("error: surface %lld is not a Forbes row of the case / bad wavelength index\n",
           (long long)s);
    return false;
  }
  return true;
}

// forbes_trace_kernel (forbes.hip) for every ray
template <typename T>
int step(const Case& c, const ol::SystemView& v) {
  using namespace ol;
  if (!forbes_row(c, v)) return 1;
  return host::run_step<T>(
      c, v, (int32_t)c.h[6],
      [](const SingleArgs<T>& a, const Ray<T>& r) {
        return forbes_step<T>(single_fetched(a), as_const(a.coeffs), r);
      },
      [](const Ray<T>& g) { return g.L != g.L && g.x == g.x; });
}

// geometry.sag(x, y) and geometry._surface_normal(x, y) (geometry.py:288-309, 573-594)
template <typename T>
int grid(const Case& c, const ol::SystemView& v) {
  using namespace ol;
  if (!forbes_row(c, v)) return 1;
  const Rows<T> t = rows_of<T>(v);
  const int64_t s = c.h[5];
  const SurfFetched<T> h{as_const(t.hot + s), as_const(t.cold + s),
                         as_const(t.opt + (s * v.n_wl + c.h[6]))};
  for (int64_t i = 0; i < c.h[4]; ++i) {
    const DevSurf<T> S = h.surf();
    T sag, fx, fy;
    forbes_eval<T>(S, as_const(t.coeffs) + S.coeff_off, (T)c.plane[0][i], (T)c.plane[1][i], sag, fx,
                   fy);
    const double mag = std::sqrt((double)fx * fx + (double)fy * fy + 1.0);
    printf("pt %lld %.17g %.17g %.17g %.17g\n", (long long)i, (double)sag, fx / mag, fy / mag,
           -1.0 / mag);
  }
  return 0;
}

// ol_trace_forbes's own rules, then the precedence: the first broken rule answers
int rules(Case& c, ol_system* sys) {
  const int32_t wl = (int32_t)c.h[6], s = (int32_t)c.h[5], n_surf = (int32_t)c.h[1];
  const int64_t n = c.h[4];
  const auto check = host::rules(kProgram, c, sys, wl);
  say("all at once", check(sys, (ol_dtype)5, -1, nullptr, -1, 0.0, nullptr, 0, n_surf, ~0u));
  say("all but dtype", check(sys, OL_F64, -1, nullptr, -1, 0.0, nullptr, 0, n_surf, ~0u));
  say("surface before wavelength", check(sys, OL_F64, n, nullptr, -1, 0.0, nullptr, 0, n_surf, ~0u));
  say("wavelength before flags", check(sys, OL_F64, n, nullptr, -1, 0.0, nullptr, 0, s, ~0u));
  say("flags before planes", check(sys, OL_F64, n, nullptr, wl, 0.0, nullptr, 0, s, ~0u));
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  return host::main_of(kProgram, argc, argv,
                       [](const char* mode, Case& c, ol_system* sys, const ol::SystemView& v) {
    if (strcmp(mode, "step") == 0) return c.h[7] ? step<double>(c, v) : step<float>(c, v);
    if (strcmp(mode, "grid") == 0) return c.h[7] ? grid<double>(c, v) : grid<float>(c, v);
    if (strcmp(mode, "refuse") == 0) return host::refuse(c, sys, (int32_t)c.h[6], true);
    return rules(c, sys);
  });
}
