// ensemble_rules.h -- what an ol_ensemble asks of its variants, each rule stated ONCE in the manner
// of entry_rules.h: a function of (who, ...) that returns OL_OK or the code of the broken rule,
// its text in ol_last_error.  optiland_amd/ensemble.py applies the same rules to packed tables
// with the same texts before anything reaches the library, and the tests match on them.
//
// The variants of an ensemble share ONE kernel instantiation, one launch grid and one set of
// table strides, so they must agree in everything that selects code or layout; values are free.
// Host-only and header-only.
#pragma once

#include <stdint.h>

#include <vector>

#include "../../include/optiland_hip.h"
#include "entry_rules.h"
#include "last_error.h"
#include "system_stage.h"

namespace ol {

// OL_SURF_ROTATED states what rot[] holds -- a tilt tolerance sets it on one variant and not on
// the nominal lens -- and is a run-time branch on the variant's own row; the other flags select
// arithmetic (OL_SURF_REFERENCE_ROOT) or a kernel family (OL_SURF_REFERENCE_NEWTON)
constexpr uint32_t kEnsembleFlagMask = ~(uint32_t)OL_SURF_ROTATED;

// the public rows of variant `k` against variant 0's: the first differing field of the first
// differing surface answers
inline int rule_same_rows(const char* who, int32_t k, const ol_surface_desc* ref, int32_t ref_coeffs,
                          const ol_surface_desc* var, int32_t var_coeffs, int32_t n_surf) {
  for (int32_t s = 0; s < n_surf; ++s) {
    const ol_surface_desc &a = ref[s], &b = var[s];
    const struct { const char* name; int64_t want, got; } fields[] = {
        {"geom_kind", a.geom_kind, b.geom_kind},
        {"interaction", a.interaction, b.interaction},
        {"aperture_kind", a.aperture_kind, b.aperture_kind},
        {"coating_kind", a.coating_kind, b.coating_kind},
        {"flags", (int64_t)(a.flags & kEnsembleFlagMask), (int64_t)(b.flags & kEnsembleFlagMask)},
        {"n_coeff", a.n_coeff, b.n_coeff},
        {"coeff_offset", a.coeff_offset, b.coeff_offset},
        {"poly_cols", a.poly_cols, b.poly_cols},
    };
    for (const auto& f : fields)
      if (f.want != f.got)
        return failf(OL_EINVAL, "%s: variant %d, surface %d: %s %lld differs from variant 0's %lld "
                                "(the variants of an ensemble share their structure)", who, k, s,
                     f.name, (long long)f.got, (long long)f.want);
  }
  if (ref_coeffs != var_coeffs)
    return failf(OL_EINVAL, "%s: variant %d: coefficient buffer of %d values differs from variant "
                            "0's %d (the variants of an ensemble share their structure)", who, k,
                 var_coeffs, ref_coeffs);
  return OL_OK;
}

// ... and the STAGED rows: the layout of the device coefficient blocks (a Zernike surface is staged
// in one of two forms by its values) and the Newton family of the whole system
inline int rule_same_staging(const char* who, int32_t k, const Staged& ref, const Staged& var) {
  for (size_t s = 0; s < ref.surf.size(); ++s) {
    const HostSurf &a = ref.surf[s], &b = var.surf[s];
    const struct { const char* name; int64_t want, got; } fields[] = {
        {"staged geometry", a.geom, b.geom},
        {"staged n_coeff", a.n_coeff, b.n_coeff},
        {"staged coefficient offset", a.coeff_off, b.coeff_off},
        {"staged coefficient count", a.coeff_len, b.coeff_len},
        {"staged aperture tokens", a.ap_len, b.ap_len},
    };
    for (const auto& f : fields)
      if (f.want != f.got)
        return failf(OL_EINVAL, "%s: variant %d, surface %d: %s %lld differs from variant 0's %lld "
                                "(the variants of an ensemble share their structure)", who, k,
                     (int)s, f.name, (long long)f.got, (long long)f.want);
  }
  if (ref.coeffs.size() != var.coeffs.size())
    return failf(OL_EINVAL, "%s: variant %d: %zu staged coefficients differ from variant 0's %zu "
                            "(the variants of an ensemble share their structure)", who, k,
                 var.coeffs.size(), ref.coeffs.size());
  return OL_OK;
}

// a view of staged facts for the rules of entry_rules.h that read a SystemView's host copies
// (no device table behind it)
inline SystemView facts_view(const HostFacts& f, int32_t n_surf, int32_t n_wl, int device) {
  SystemView v{};
  v.n_surf = n_surf;
  v.n_wl = n_wl;
  v.device = device;
  v.consistent = true;
  v.interaction = f.interaction.data();
  v.coating = f.coating.data();
  v.ref_newton = f.ref_newton.data();
  v.geom = f.geom.data();
  return v;
}

inline int rule_ensemble(const char* who, const ol_ensemble* ens) {
  return ens ? OL_OK : failf(OL_EINVAL, "%s: ensemble is NULL", who);
}

inline int rule_variant_range(const char* who, int32_t k0, int32_t count, int32_t size) {
  if (k0 >= 0 && count >= 0 && (int64_t)k0 + count <= size) return OL_OK;
  return failf(OL_EINVAL, "%s: variants [%d, %d + %d) outside [0, %d)", who, k0, k0, count, size);
}

inline int rule_variant_record(const char* who, int32_t k, const ol_ensemble_variant& v) {
  if (v.surf && v.optics && v.raygen && v.n_coeffs >= 0 && (v.n_coeffs == 0 || v.coeffs))
    return OL_OK;
  return failf(OL_EINVAL, "%s: variant %d: NULL table, optics or raygen (or a bad coefficient "
                          "buffer)", who, k);
}

// the ray generator's launch-invariant switches are structure too (RaygenConsts: they pick
// branches every lane takes alike, and the apodization a kernel instantiation)
inline int rule_same_raygen(const char* who, int32_t k, const ol_raygen_params& a,
                            const ol_raygen_params& b) {
  const struct { const char* name; int64_t want, got; } fields[] = {
      {"object_infinite", a.object_infinite != 0, b.object_infinite != 0},
      {"field_kind", a.field_kind, b.field_kind},
      {"apod_kind", a.apod_kind, b.apod_kind},
      {"telecentric", a.tele_dz > 0.0, b.tele_dz > 0.0},
  };
  for (const auto& f : fields)
    if (f.want != f.got)
      return failf(OL_EINVAL, "%s: variant %d: raygen %s %lld differs from variant 0's %lld (the "
                              "variants of an ensemble share their structure)", who, k, f.name,
                   (long long)f.got, (long long)f.want);
  return OL_OK;
}

}  // namespace ol
