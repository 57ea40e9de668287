// main.hip -- TEST INFRASTRUCTURE: the cell walk of optiland_amd/csrc/ensemble_device.h compiled
// for the host (OL_HOST_MATH) and run cell by cell, ray by ray, as a stand-alone program.
//
//   hostensemble walk <case file>    ensemble_spot_kernel's body for every cell: the stacked tables
//                                    built as ensemble.hip builds them (system_stage.h,
//                                    table_image.h), then per cell the variant lookup, the field
//                                    point, the generated ray and the surface walk of
//                                    ensemble_device.h; one line per ray, then the status word
//   hostensemble alone <case file>   every cell as ONE variant alone: ol_system_create of that
//                                    variant and ol_trace_spot with per-ray field planes (the host
//                                    build of csrc/capi.hip); the same lines
//   hostensemble check <case file>   the structure rules of csrc/ensemble_rules.h on the case's
//                                    variants: return code and message
//
// Linked with the host-only compile of csrc/capi.hip and tests/hostmath/harness.hip (the objects
// tests/hostmath/build.py leaves behind), plain or with AddressSanitizer +
// UndefinedBehaviorSanitizer.  A program of its own: nothing is loaded into an interpreter.  Not a
// fallback: nothing under optiland_amd/ knows about it.
//
// Case file (little endian): 8 int64 -- magic, K, n_surf, n_wl, n_coeff, n rays, n cells, dtype
// (0 = fp32, 1 = fp64); per variant n_surf ol_surface_desc, n_surf x n_wl ol_surface_optics,
// n_coeff doubles, one ol_raygen_params; px and py (n doubles each); n cells ol_ensemble_cell.
#define OL_HOST_MATH 1
#include "../../optiland_amd/csrc/ensemble_device.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/optiland_hip.h"
#include "../../optiland_amd/csrc/ensemble_rules.h"
#include "../../optiland_amd/csrc/system_stage.h"
#include "../../optiland_amd/csrc/table_image.h"

namespace {

constexpr int64_t kMagic = 0x534e456c6fLL;  // "olENS"

struct Variant {
  std::vector<ol_surface_desc> surf;
  std::vector<ol_surface_optics> optics;
  std::vector<double> coeffs;
  ol_raygen_params raygen;
};

struct Case {
  int64_t h[8];
  std::vector<Variant> variants;
  std::vector<double> px, py;
  std::vector<ol_ensemble_cell> cells;
};

bool read_exact(FILE* f, void* dst, size_t bytes) { return bytes == 0 || fread(dst, bytes, 1, f) == 1; }

bool load(const char* path, Case& c) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  bool ok = read_exact(f, c.h, sizeof c.h) && c.h[0] == kMagic;
  // sizes a case file of this suite stays far inside: a corrupt header must not allocate
  ok = ok && c.h[1] > 0 && c.h[1] < 4096 && c.h[2] > 0 && c.h[2] < 4096 && c.h[3] > 0 &&
       c.h[3] < 64 && c.h[4] >= 0 && c.h[4] < (1 << 24) && c.h[5] >= 0 && c.h[5] < (1 << 24) &&
       c.h[6] >= 0 && c.h[6] < (1 << 24);
  if (ok) {
    const size_t ns = (size_t)c.h[2], nw = (size_t)c.h[3], nc = (size_t)c.h[4];
    c.variants.resize((size_t)c.h[1]);
    for (Variant& v : c.variants) {
      v.surf.resize(ns);
      v.optics.resize(ns * nw);
      v.coeffs.resize(nc);
      ok = ok && read_exact(f, v.surf.data(), ns * sizeof(ol_surface_desc)) &&
           read_exact(f, v.optics.data(), ns * nw * sizeof(ol_surface_optics)) &&
           read_exact(f, v.coeffs.data(), nc * sizeof(double)) &&
           read_exact(f, &v.raygen, sizeof v.raygen);
    }
    c.px.resize((size_t)c.h[5]);
    c.py.resize((size_t)c.h[5]);
    c.cells.resize((size_t)c.h[6]);
    ok = ok && read_exact(f, c.px.data(), c.px.size() * sizeof(double)) &&
         read_exact(f, c.py.data(), c.py.size() * sizeof(double)) &&
         read_exact(f, c.cells.data(), c.cells.size() * sizeof(ol_ensemble_cell));
  }
  fclose(f);
  return ok;
}

ol::RaygenDev raygen_of(const ol_raygen_params& g) {
  return ol::RaygenDev{g.object_infinite, g.field_kind, g.EPL,     g.EPD,    g.max_field,
                       g.offset,          g.z_first,    g.tele_dz, g.apod_a, g.apod_b,
                       g.apod_kind};
}

void say_ray(int64_t c, int64_t j, double x, double y, double i) {
  printf("cell %lld ray %lld %.17g %.17g %.17g\n", (long long)c, (long long)j, x, y, i);
}

int stage_all(const Case& c, std::vector<ol::Staged>& st) {
  st.assign(c.variants.size(), ol::Staged());
  for (size_t k = 0; k < c.variants.size(); ++k) {
    const Variant& v = c.variants[k];
    if (int rc = ol::stage_system("hostensemble", v.surf.data(), (int32_t)c.h[2],
                                  v.coeffs.empty() ? nullptr : v.coeffs.data(),
                                  (int32_t)v.coeffs.size(), v.optics.data(), (int32_t)c.h[3], st[k]))
      return rc;
  }
  return OL_OK;
}

// the structure rules, variant by variant against variant 0, as ol_ensemble_create applies them
int check(const Case& c) {
  std::vector<ol::Staged> st;
  int rc = stage_all(c, st);
  const Variant& v0 = c.variants[0];
  if (rc == OL_OK)
    rc = ol::rule_no_reference_newton(
        "ol_ensemble_create", ol::facts_view(st[0].facts, (int32_t)c.h[2], (int32_t)c.h[3], 0));
  for (size_t k = 1; rc == OL_OK && k < c.variants.size(); ++k) {
    const Variant& v = c.variants[k];
    rc = ol::rule_same_rows("ol_ensemble_create", (int32_t)k, v0.surf.data(),
                            (int32_t)v0.coeffs.size(), v.surf.data(), (int32_t)v.coeffs.size(),
                            (int32_t)c.h[2]);
    if (rc == OL_OK) rc = ol::rule_same_raygen("ol_ensemble_create", (int32_t)k, v0.raygen, v.raygen);
    if (rc == OL_OK) rc = ol::rule_same_staging("ol_ensemble_create", (int32_t)k, st[0], st[k]);
  }
  printf("check: %d %s\n", rc, rc ? ol_last_error() : "ok");
  return 0;
}

template <typename T, int NR>
int walk_nr(const Case& c, const std::vector<ol::Staged>& st) {
  using namespace ol;
  const size_t K = st.size(), ns = (size_t)c.h[2], no = ns * (size_t)c.h[3];
  const size_t cap = st[0].coeffs.size() ? st[0].coeffs.size() : 1;
  std::vector<DevSurfHot<T>> surf(K * ns);
  std::vector<DevSurfCold<T>> cold(K * ns);
  std::vector<DevOptics<T>> optics(K * no);
  std::vector<T> coeffs(K * cap, T(0));
  std::vector<RaygenConsts<T>> rgc(K);
  for (size_t k = 0; k < K; ++k) {
    if (st[k].coeffs.size() > cap) {
      printf("error: variant %zu stages %zu coefficients, variant 0 %zu\n", k, st[k].coeffs.size(),
             cap);
      return 1;
    }
    write_table_image<T>(st[k].surf, st[k].optics, st[k].coeffs, st[k].int_slots,
                         surf.data() + k * ns, cold.data() + k * ns, optics.data() + k * no,
                         coeffs.data() + k * cap);
    rgc[k] = RaygenConsts<T>(raygen_of(c.variants[k].raygen));
  }
  const EnsembleTables<T> tab{surf.data(), cold.data(), optics.data(), coeffs.data(), rgc.data(),
                              (int32_t)K,  (int32_t)ns, (int32_t)c.h[3], (int32_t)cap};
  const bool apod = c.variants[0].raygen.apod_kind != 0;
  uint32_t status = 0;
  for (size_t ci = 0; ci < c.cells.size(); ++ci) {
    const ol_ensemble_cell* cell = &c.cells[ci];
    if (!ensemble_cell_ok(tab, cell->variant, cell->wavelength_index)) {
      status |= kStatusEnsembleCell;
      continue;
    }
    const EnsembleRows<T> rows = ensemble_rows(tab, cell->variant, cell->wavelength_index);
    const RaygenConsts<T> k = load_consts(rows.rgc);
    const EnsembleField<T> f = ensemble_field<T>(k, cell, 0u, status);
    for (size_t j = 0; j < c.px.size(); ++j) {
      T px = (T)c.px[j], py = (T)c.py[j], o[6];
      raygen_pupil<T>(0u, f.vx, f.vy, px, py, status);
      raygen_one<T>(k, f.tx, f.ty, px, py, f.vx, f.vy, o);
      Ray<T> r[1], g[1];
      r[0].x = o[0]; r[0].y = o[1]; r[0].z = o[2];
      r[0].L = o[3]; r[0].M = o[4]; r[0].N = o[5];
      r[0].i = apod ? raygen_apodize<T>(k, px, py) : T(1);
      r[0].opd = T(0);
      ensemble_walk<T, T, 1, NR, false, false>(rows, (int)ns, (int)c.h[3], false, r, g, status);
      say_ray((int64_t)ci, (int64_t)j, (double)g[0].x, (double)g[0].y, (double)g[0].i);
    }
  }
  printf("status %u\n", status);
  return 0;
}

template <typename T>
int walk(const Case& c) {
  std::vector<ol::Staged> st;
  if (int rc = stage_all(c, st)) {
    printf("error: staging: %d %s\n", rc, ol_last_error());
    return 1;
  }
  switch (ol::newton_family_of(st[0].facts, 0, (int32_t)c.h[2] - 1)) {
    case ol::kNrNone: return walk_nr<T, ol::kNrNone>(c, st);
    case ol::kNrZernike: return walk_nr<T, ol::kNrZernike>(c, st);
    case ol::kNrEvenAsphere: return walk_nr<T, ol::kNrEvenAsphere>(c, st);
    default: return walk_nr<T, ol::kNrGeneric>(c, st);
  }
}

// every cell through ol_trace_spot on a system of its variant alone, per-ray field planes
template <typename T>
int alone(const Case& c) {
  const size_t n = c.px.size();
  std::vector<T> px(c.px.begin(), c.px.end()), py(c.py.begin(), c.py.end()), hx(n), hy(n), x(n),
      y(n), inten(n);
  uint32_t status = 0;
  for (size_t ci = 0; ci < c.cells.size(); ++ci) {
    const ol_ensemble_cell& cell = c.cells[ci];
    if (cell.variant < 0 || cell.variant >= (int32_t)c.variants.size()) continue;
    const Variant& v = c.variants[(size_t)cell.variant];
    ol_system* sys = nullptr;
    int rc = ol_system_create(v.surf.data(), (int32_t)c.h[2],
                              v.coeffs.empty() ? nullptr : v.coeffs.data(), (int32_t)v.coeffs.size(),
                              v.optics.data(), (int32_t)c.h[3], &sys);
    if (rc != OL_OK) {
      printf("error: ol_system_create: %s\n", ol_last_error());
      return 1;
    }
    for (size_t j = 0; j < n; ++j) { hx[j] = (T)cell.hx; hy[j] = (T)cell.hy; }
    ol_raygen_inputs in{};
    in.px = px.data(); in.py = py.data(); in.hx = hx.data(); in.hy = hy.data();
    in.vx0 = cell.vx; in.vy0 = cell.vy;
    void* hits[3] = {x.data(), y.data(), inten.data()};
    double out7[8] = {0};
    rc = ol_trace_spot(sys, sizeof(T) == 4 ? OL_F32 : OL_F64, (int64_t)n, &v.raygen, &in, cell.cx,
                       cell.cy, cell.wavelength_index, hits, out7, &status, nullptr);
    ol_system_destroy(sys);
    if (rc != OL_OK) {
      printf("error: ol_trace_spot: %s\n", ol_last_error());
      return 1;
    }
    for (size_t j = 0; j < n; ++j)
      say_ray((int64_t)ci, (int64_t)j, (double)x[j], (double)y[j], (double)inten[j]);
  }
  printf("status %u\n", status);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const bool known = argc == 3 && (!strcmp(argv[1], "walk") || !strcmp(argv[1], "alone") ||
                                   !strcmp(argv[1], "check"));
  if (!known) {
    fprintf(stderr, "usage: hostensemble walk|alone|check <case file>\n");
    return 2;
  }
  Case c;
  if (!load(argv[2], c)) {
    fprintf(stderr, "hostensemble: cannot read the case file %s\n", argv[2]);
    return 2;
  }
  if (!strcmp(argv[1], "check")) return check(c);
  if (!strcmp(argv[1], "walk")) return c.h[7] ? walk<double>(c) : walk<float>(c);
  return c.h[7] ? alone<double>(c) : alone<float>(c);
}
