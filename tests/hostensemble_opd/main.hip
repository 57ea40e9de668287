// main.hip -- TEST INFRASTRUCTURE: the wavefront cells of optiland_amd/csrc/ensemble_opd_device.h
// compiled for the host (OL_HOST_MATH) and run cell by cell, ray by ray, as a stand-alone program.
//
//   hostensemble_opd walk <case file>   the two kernels of csrc/ensemble_opd.hip for every cell:
//                                       the stacked tables built as ensemble.hip builds them
//                                       (system_stage.h, table_image.h), then per cell the chief
//                                       ray -> its reference (ensemble_chief_kernel's body), and
//                                       per ray the OPD against it (ensemble_opd_kernel's body)
//                                       and the twelve moments.  Printed: one `ref` line per cell
//                                       (the 15 values of the reference and its planar flag), one
//                                       `ray` line per ray (OPD in waves, intensity, pupil
//                                       point), one `mom` line per cell, then the status word.  A
//                                       cell the ensemble does not hold prints nothing.
//
// Linked with the host-only compile of csrc/capi.hip and tests/hostmath/harness.hip (the objects
// tests/hostmath/build.py leaves behind), plain or with AddressSanitizer +
// UndefinedBehaviorSanitizer.  A program of its own: nothing is loaded into an interpreter.  Not a
// fallback: nothing under optiland_amd/ knows about it.
//
// Case file (little endian): 8 int64 -- magic, K, n_surf, n_wl, n_coeff, n rays, n cells, raygen
// flags; per variant n_surf ol_surface_desc, n_surf x n_wl ol_surface_optics, n_coeff doubles, one
// ol_raygen_params; px and py (n doubles each); n cells ol_ensemble_opd_cell.
#define OL_HOST_MATH 1
#include "../../optiland_amd/csrc/ensemble_opd_device.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/optiland_hip.h"
#include "../../optiland_amd/csrc/ensemble_rules.h"
#include "../../optiland_amd/csrc/epilogue_device.h"
#include "../../optiland_amd/csrc/system_stage.h"
#include "../../optiland_amd/csrc/table_image.h"

namespace {

constexpr int64_t kMagic = 0x44504f6c6fLL;  // "olOPD"

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
  std::vector<ol_ensemble_opd_cell> cells;
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
         read_exact(f, c.cells.data(), c.cells.size() * sizeof(ol_ensemble_opd_cell));
  }
  fclose(f);
  return ok;
}

ol::RaygenDev raygen_of(const ol_raygen_params& g) {
  return ol::RaygenDev{g.object_infinite, g.field_kind, g.EPL,     g.EPD,    g.max_field,
                       g.offset,          g.z_first,    g.tele_dz, g.apod_a, g.apod_b,
                       g.apod_kind};
}

template <int NR, bool APOD>
int walk_nr(const Case& c, const std::vector<ol::Staged>& st) {
  using namespace ol;
  using T = double;
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
  const uint32_t flags = (uint32_t)c.h[7];
  uint32_t status = 0;
  for (size_t ci = 0; ci < c.cells.size(); ++ci) {
    const ol_ensemble_opd_cell* cell = &c.cells[ci];
    if (!ensemble_cell_ok(tab, cell->variant, cell->wavelength_index)) {
      status |= kStatusEnsembleCell;
      continue;
    }
    const EnsembleRows<T> rows = ensemble_rows(tab, cell->variant, cell->wavelength_index);
    // the chief-ray launch (cold: the generic Newton instantiation serves every family)
    const WavefrontConsts<T> w =
        opd_cell_chief<(NR == kNrNone ? kNrNone : kNrGeneric)>(rows, (int)ns, (int)c.h[3], cell,
                                                               flags, status);
    printf("ref %zu %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g "
           "%.17g %.17g %d\n", ci, w.xc, w.yc, w.zc, w.R, w.ni, w.inv_w, w.ux, w.uy, w.half_epd,
           w.opd_ref, w.nx, w.ny, w.nz, w.last_t, w.last_absorb, (int)w.planar);
    // the OPD launch
    const OpdCellField f = opd_cell_field(load_consts(rows.rgc), cell, flags, status);
    double s[kOpdMoments] = {0};
    for (size_t j = 0; j < c.px.size(); ++j) {
      double ov, gi, pu[3];
      opd_cell_trace<NR, APOD, false>(rows, (int)ns, (int)c.h[3], f, flags, &w, c.px[j], c.py[j],
                                      status, ov, gi, pu);
      opd_accumulate(s, gi, ov, pu[0], pu[1], gi > 0.0);
      printf("ray %zu %zu %.17g %.17g %.17g %.17g %.17g\n", ci, j, ov, gi, pu[0], pu[1], pu[2]);
    }
    printf("mom %zu", ci);
    for (int k = 0; k < kOpdMoments; ++k) printf(" %.17g", s[k]);
    printf("\n");
  }
  printf("status %u\n", status);
  return 0;
}

int walk(const Case& c) {
  std::vector<ol::Staged> st(c.variants.size());
  for (size_t k = 0; k < c.variants.size(); ++k) {
    const Variant& v = c.variants[k];
    if (int rc = ol::stage_system("hostensemble_opd", v.surf.data(), (int32_t)c.h[2],
                                  v.coeffs.empty() ? nullptr : v.coeffs.data(),
                                  (int32_t)v.coeffs.size(), v.optics.data(), (int32_t)c.h[3],
                                  st[k])) {
      printf("error: staging: %d %s\n", rc, ol_last_error());
      return 1;
    }
  }
  const bool apod = c.variants[0].raygen.apod_kind != 0;
#define OL_WALK(N) (apod ? walk_nr<N, true>(c, st) : walk_nr<N, false>(c, st))
  switch (ol::newton_family_of(st[0].facts, 0, (int32_t)c.h[2] - 1)) {
    case ol::kNrNone: return OL_WALK(ol::kNrNone);
    case ol::kNrZernike: return OL_WALK(ol::kNrZernike);
    case ol::kNrEvenAsphere: return OL_WALK(ol::kNrEvenAsphere);
    default: return OL_WALK(ol::kNrGeneric);
  }
#undef OL_WALK
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3 || strcmp(argv[1], "walk")) {
    fprintf(stderr, "usage: hostensemble_opd walk <case file>\n");
    return 2;
  }
  Case c;
  if (!load(argv[2], c)) {
    fprintf(stderr, "hostensemble_opd: cannot read the case file %s\n", argv[2]);
    return 2;
  }
  return walk(c);
}
