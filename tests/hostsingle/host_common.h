// host_common.h -- TEST INFRASTRUCTURE: what the stand-alone programs of tests/hostforbes,
// hostgrating, hostphase and hostgrid share -- the case file, the `step` loop over the product's
// own ray I/O (csrc/single_surface.h), the `refuse` list, the shared part of `rules` and `main`.
// Each program keeps its file layout, its modes and its printed lines.
//
// Case file (little endian): 8 int64 -- magic, n_surf, n_wl, n_coeff, n, surface, h[6], dtype
// (0 = fp32, 1 = fp64); [one double -- the wavelength in micrometres;] then n_surf
// ol_surface_desc, n_surf x n_wl ol_surface_optics, n_coeff doubles, 8 planes of n doubles (x, y,
// z, L, M, N, i, opd) [, h[6] probe doubles].  h[6] is the wavelength index, or the number of
// probes.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/optiland_hip.h"
#include "../../optiland_amd/csrc/ray_aim_host.h"
#include "../../optiland_amd/csrc/single_surface.h"

namespace host {

struct Program {
  const char* name;           // "hostforbes"
  const char* modes;          // "step|grid|refuse|create|rules", as the usage line prints them
  int64_t magic;
  int kind;                   // its row of ol::kSingleKinds
  bool wavelength;            // the wavelength follows the header
  bool probes;                // h[6] counts probe coordinates behind the planes (else: wl index)
  const char* not_a_row;      // the label of the `rules` line on the row behind the surface
};

struct Case {
  int64_t h[8];
  double wavelength = 0.0;
  std::vector<ol_surface_desc> surf;
  std::vector<ol_surface_optics> optics;
  std::vector<double> coeffs, plane[8], probe;
};

inline bool read_exact(FILE* f, void* dst, size_t bytes) {
  return bytes == 0 || fread(dst, bytes, 1, f) == 1;
}

inline bool load(const Program& p, const char* path, Case& c) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  bool ok = read_exact(f, c.h, sizeof c.h) && c.h[0] == p.magic &&
            (!p.wavelength || read_exact(f, &c.wavelength, sizeof c.wavelength));
  // sizes a case file of this suite stays far inside: a corrupt header must not allocate
  ok = ok && c.h[1] > 0 && c.h[1] < 4096 && c.h[2] > 0 && c.h[2] < 64 && c.h[3] >= 0 &&
       c.h[3] < (1 << 24) && c.h[4] >= 0 && c.h[4] < (1 << 24) &&
       (!p.probes || (c.h[6] >= 0 && c.h[6] < (1 << 24)));
  if (ok) {
    const size_t ns = (size_t)c.h[1], nw = (size_t)c.h[2], nc = (size_t)c.h[3], n = (size_t)c.h[4];
    c.surf.resize(ns);
    c.optics.resize(ns * nw);
    c.coeffs.resize(nc);
    ok = read_exact(f, c.surf.data(), ns * sizeof(ol_surface_desc)) &&
         read_exact(f, c.optics.data(), ns * nw * sizeof(ol_surface_optics)) &&
         read_exact(f, c.coeffs.data(), nc * sizeof(double));
    for (auto& q : c.plane) {
      q.resize(n);
      ok = ok && read_exact(f, q.data(), n * sizeof(double));
    }
    if (p.probes) {
      c.probe.resize((size_t)c.h[6]);
      ok = ok && read_exact(f, c.probe.data(), c.probe.size() * sizeof(double));
    }
  }
  fclose(f);
  return ok;
}

inline void say(const char* what, int rc) {
  printf("%s: %d %s\n", what, rc, rc ? ol_last_error() : "ok");
}

// The kernel's body for every ray, a "wave" of one ray each: the case's planes in T, the
// product's single_args / single_load / single_store on them with a recorded row AND the
// write-back, `step(a, r)` in between (the program's *_step on single_fetched(a)), `lost(g)`
// the per-ray part of its kernel's status rule.  One line per ray, from what the stores wrote.
template <typename T, typename Step, typename Lost>
int run_step(const Case& c, const ol::SystemView& v, int32_t wl, Step step, Lost lost) {
  using namespace ol;
  const int64_t n = c.h[4];
  std::vector<T> planes[8], row(8 * (size_t)n);
  void* rays[8];
  for (int k = 0; k < 8; ++k) {
    planes[k].assign(c.plane[k].begin(), c.plane[k].end());
    rays[k] = planes[k].data();
  }
  const SingleArgs<T> a = single_args<T>(v, (int32_t)c.h[5], wl, n, rays, row.data(), n,
                                         kTraceWriteRays, nullptr);
  std::vector<uint32_t> bits((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    const Ray<T> g = step(a, single_load(a, i));
    single_store(a, i, g);
    bits[i] = lost(g) ? OL_STATUS_NAN_DIRECTION : 0u;
  }
  for (int64_t i = 0; i < n; ++i) {
    const T* p = row.data() + i;
    for (int k = 0; k < 8; ++k)
      if (memcmp(&p[k * n], &planes[k][i], sizeof(T)) != 0) {
        printf("error: ray %lld: the state written back is not the recorded row\n", (long long)i);
        return 1;
      }
    printf("ray %lld %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %u\n", (long long)i,
           (double)p[0], (double)p[n], (double)p[2 * n], (double)p[3 * n], (double)p[4 * n],
           (double)p[5 * n], (double)p[6 * n], (double)p[7 * n], bits[i]);
  }
  return 0;
}

// every entry point that walks a surface range, on a range that holds the case's row:
// OL_EUNSUPPORTED before anything is launched (the arguments behind the range are never read).
// `before_the_row`: also the range in front of the row, which is an ordinary one
inline int refuse(const Case& c, ol_system* sys, int32_t wl, bool before_the_row) {
  const int32_t last = (int32_t)c.h[1] - 1, s = (int32_t)c.h[5];
  double plane[4] = {0, 0, 0, 0};
  void* rays[8] = {plane, plane, plane, plane, plane, plane, plane, plane};
  uint32_t status = 0;
  int32_t iters[8192] = {0};
  ol_raygen_params rg{};
  ol_raygen_inputs in{};
  in.px = plane;
  in.py = plane;
  say("ol_trace", ol_trace(sys, OL_F64, 1, rays, wl, nullptr, 0, nullptr, 0, last,
                           OL_TRACE_WRITE_RAYS, &status, nullptr));
  say("ol_trace one surface", ol_trace(sys, OL_F32, 1, rays, wl, nullptr, 0, nullptr, s, s,
                                       OL_TRACE_WRITE_RAYS, &status, nullptr));
  say("ol_trace_ex", ol_trace_ex(sys, OL_F64, 1, rays, wl, nullptr, 0, nullptr, 0, last,
                                 OL_TRACE_WRITE_RAYS, &status, nullptr, nullptr));
  if (before_the_row)
    say("ol_trace before the row", s > 1 ? ol_trace(sys, OL_F64, 1, rays, wl, nullptr, 0, nullptr,
                                                    0, s - 1, OL_TRACE_WRITE_RAYS, &status,
                                                    nullptr)
                                         : 0);
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

// The entry's own rules (csrc/single_host.h), one broken at a time (every plane is a real one of
// the case); a program adds its lines on the precedence of the rules behind these.
// `check(sys, dt, n, rays, wl, wavelength_um, row, stride, surface, flags)`: single_check for the
// program's kind, returned for those lines.
inline auto rules(const Program& p, Case& c, ol_system* sys, int32_t wl) {
  const ol::SingleKind& kind = ol::kSingleKinds[p.kind];
  auto check = [&kind](const ol_system* sy, ol_dtype dt, int64_t n, void* const rays[8],
                       int32_t wli, double w, const void* row, int64_t stride, int32_t s,
                       uint32_t flags) {
    return ol::single_check(kind, sy, dt, n, rays, wli, kind.takes_wavelength_um ? &w : nullptr,
                            row, stride, s, flags);
  };
  const int32_t s = (int32_t)c.h[5], n_surf = (int32_t)c.h[1];
  const int64_t n = c.h[4];
  const double w = c.wavelength;
  std::vector<double> row(8 * (size_t)n + 1);
  void* rays[8];
  for (int k = 0; k < 8; ++k) rays[k] = c.plane[k].data();
  const uint32_t wr = OL_TRACE_WRITE_RAYS;
  say("good", check(sys, OL_F64, n, rays, wl, w, row.data(), n, s, 0));
  say("good fp32 midrange", check(sys, OL_F32, n, rays, wl, w, nullptr, 0, s,
                                  wr | OL_TRACE_MIDRANGE));
  say("empty", check(sys, OL_F64, 0, nullptr, wl, w, nullptr, 0, s, 0));
  say("null system", check(nullptr, OL_F64, n, rays, wl, w, row.data(), n, s, 0));
  say("dtype", check(sys, (ol_dtype)5, n, rays, wl, w, row.data(), n, s, 0));
  say("negative count", check(sys, OL_F64, -1, rays, wl, w, row.data(), n, s, 0));
  say("surface -1", check(sys, OL_F64, n, rays, wl, w, row.data(), n, -1, 0));
  say("surface past the table", check(sys, OL_F64, n, rays, wl, w, row.data(), n, n_surf, 0));
  say(p.not_a_row, check(sys, OL_F64, n, rays, wl, w, row.data(), n, s + 1, 0));
  say("wavelength", check(sys, OL_F64, n, rays, (int32_t)c.h[2], w, row.data(), n, s, 0));
  say("wavelength -1", check(sys, OL_F64, n, rays, -1, w, row.data(), n, s, 0));
  if (kind.takes_wavelength_um) {
    say("wavelength_um 0", check(sys, OL_F64, n, rays, wl, 0.0, row.data(), n, s, 0));
    say("wavelength_um negative", check(sys, OL_F64, n, rays, wl, -0.5, row.data(), n, s, 0));
    say("wavelength_um inf", check(sys, OL_F64, n, rays, wl,
                                   std::numeric_limits<double>::infinity(), row.data(), n, s, 0));
    say("wavelength_um nan", check(sys, OL_F64, n, rays, wl,
                                   std::numeric_limits<double>::quiet_NaN(), row.data(), n, s, 0));
  }
  say("flags", check(sys, OL_F64, n, rays, wl, w, row.data(), n, s, OL_TRACE_PRT_COMPLEX));
  say("too many", check(sys, OL_F64, ((int64_t)0x7fffffff * 64) + 1, rays, wl, w, nullptr, 0, s,
                        wr));
  say("null rays", check(sys, OL_F64, n, nullptr, wl, w, row.data(), n, s, 0));
  { void* b[8];
    for (int k = 0; k < 8; ++k) b[k] = k == 5 ? nullptr : rays[k];
    say("null plane", check(sys, OL_F64, n, b, wl, w, row.data(), n, s, 0)); }
  say("stride", check(sys, OL_F64, n, rays, wl, w, row.data(), n - 1, s, 0));
  say("nothing to write", check(sys, OL_F64, n, rays, wl, w, nullptr, 0, s, 0));
  return check;
}

// `mode` is one of the names in p.modes
inline bool has_mode(const Program& p, const char* mode) {
  const std::string all = "|" + std::string(p.modes) + "|", one = "|" + std::string(mode) + "|";
  return one.size() > 2 && !strchr(mode, '|') && all.find(one) != std::string::npos;
}

// main: the usage line, the case, the system, `create`; every other mode is the program's:
// `run(mode, c, sys, v)` returns the exit code
template <typename Run>
int main_of(const Program& p, int argc, char** argv, Run run) {
  if (argc != 3 || !has_mode(p, argv[1])) {
    fprintf(stderr, "usage: %s %s <case file>\n", p.name, p.modes);
    return 2;
  }
  Case c;
  if (!load(p, argv[2], c)) {
    fprintf(stderr, "%s: cannot read the case file %s\n", p.name, argv[2]);
    return 2;
  }
  ol_system* sys = nullptr;
  const int rc = ol_system_create(c.surf.data(), (int32_t)c.surf.size(),
                                  c.coeffs.empty() ? nullptr : c.coeffs.data(),
                                  (int32_t)c.coeffs.size(), c.optics.data(), (int32_t)c.h[2], &sys);
  if (strcmp(argv[1], "create") == 0) {
    printf("create: %d %s\n", rc, rc ? ol_last_error() : "ok");
    ol_system_destroy(sys);
    return 0;
  }
  if (rc != OL_OK) {
    fprintf(stderr, "%s: ol_system_create: %s\n", p.name, ol_last_error());
    return 2;
  }
  const int out = run(argv[1], c, sys, ol::system_view(sys));
  ol_system_destroy(sys);
  return out;
}

}  // namespace host
