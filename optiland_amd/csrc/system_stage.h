// system_stage.h -- staging: argument validation and every host-side conversion of
// ol_system_create / ol_system_update, from the caller's table (ol_surface_desc rows, the coefficient
// buffer, the optics table) to the `Staged` image capi.hip uploads.  Pure host arithmetic on
// caller-supplied blocks: this header includes nothing of the HIP runtime and compiles alone with a
// plain C++ compiler.  What a kind IS (device number, block arithmetic, flags) is its row of
// geom_kinds.h; what its block BECOMES is its stager here, chosen by one switch (stage_block).
// The order of the checks is behaviour: a table with several faults reports the first one.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/optiland_hip.h"
#include "device_table.h"
#include "failf.h"
#include "geom_kinds.h"
#include "zernike_stage.h"

namespace ol {

// host-side staging record: every field of both device blocks, in double
struct HostSurf {
  int32_t geom, interaction, aperture_kind, coating_kind, coeff_off, n_coeff, max_iter;
  uint32_t flags;
  int32_t poly_cols, coeff_len, ap_off, ap_len;
  double cv, kp1, tol, inv_norm;
  double origin[3], rot[9], rel_off[3], rel_rot[9], ap[4], coat[2], axis[3], ret_cos, ret_sin;
  double radius, conic;
};

// what the entry points validate a call against, per surface (host copies: system_view.h)
struct HostFacts {
  std::vector<int32_t> interaction, coating, geom;   // as given
  std::vector<uint8_t> polygon;     // the surface uses a polygon aperture (top level or in a tree)
  std::vector<uint8_t> ref_newton;  // OL_SURF_REFERENCE_NEWTON on a traced Newton-Raphson surface
  // the surface keeps a polarised Zernike launch off the two-rays-per-lane form
  // (trace_kernel.hip: OL_POLZ_PAIR): a Zernike surface in the level form, a polarizer / retarder
  std::vector<uint8_t> no_pair;
};

// everything ol_system_create derives from its arguments, in double, before any device call
struct Staged {
  std::vector<HostSurf> surf;
  std::vector<DevOptics<double>> optics;
  std::vector<double> coeffs;
  std::vector<size_t> int_slots;  // coeffs entries uploaded as integer bit patterns
  HostFacts facts;
};

constexpr double kIdentity3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};

inline void mat3_mul_abt(const double* A, const double* B, double* out) {  // A * B^T
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double acc = 0;
      for (int k = 0; k < 3; ++k) acc += A[3 * i + k] * B[3 * j + k];
      out[3 * i + j] = acc;
    }
}

inline bool is_identity(const double* R) {
  return std::memcmp(R, kIdentity3, sizeof(kIdentity3)) == 0 ||
         std::equal(R, R + 9, kIdentity3);  // -0.0 == 0.0
}

// a count stored as a double: whole, not negative, at most `limit`
inline bool whole_count(double c, int64_t limit, int64_t& v) {
  if (!(c >= 0.0) || c > (double)limit || c != std::floor(c)) return false;
  v = (int64_t)c;
  return true;
}

// device form of a leaf aperture: squared radii, inverse squared semi-axes
inline void convert_aperture(int kind, const double* a, double* out) {
  out[0] = out[1] = out[2] = out[3] = 0.0;
  switch (kind) {
    case OL_AP_RADIAL:
    case OL_AP_OFFSET_RADIAL:
      out[0] = a[0] * a[0];
      out[1] = a[1] * a[1];
      out[2] = a[2];
      out[3] = a[3];
      break;
    case OL_AP_RECTANGULAR:
      for (int k = 0; k < 4; ++k) out[k] = a[k];
      break;
    case OL_AP_ELLIPTICAL:
      out[0] = 1.0 / (a[0] * a[0]);
      out[1] = 1.0 / (a[1] * a[1]);
      out[2] = a[2];
      out[3] = a[3];
      break;
    default:
      break;
  }
}

// The caller's rows and coefficient buffer, as the steps below read them.
struct StageIn {
  const ol_surface_desc* surf;
  const double* coeffs;
  int32_t n_coeffs;
};

// One row on its way into the tables: s -> d, its public block `src` (inside the buffer: the row
// checks have seen to that) -> the end of `out`.
struct StageRow {
  int32_t i;                        // the row's index, for the refusal texts
  const ol_surface_desc& s;
  HostSurf& d;
  const double* src;
  std::vector<double>& out;         // the device coefficient buffer
  std::vector<size_t>& int_slots;
};

// ---- row checks: the kinds in their ranges, the coefficient block inside the buffer
inline int check_row(int32_t i, const ol_surface_desc& s, int32_t n_coeffs, const GeomKind*& kind) {
  kind = geom_kind(s.geom_kind);
  if (!kind) return failf(OL_EUNSUPPORTED, "surface %d: geometry kind %d", i, s.geom_kind);
  if (s.interaction < OL_INTERACT_RECORD_ONLY || s.interaction > OL_INTERACT_REFLECT)
    return failf(OL_EUNSUPPORTED, "surface %d: interaction %d", i, s.interaction);
  if (s.aperture_kind < OL_AP_NONE || s.aperture_kind > OL_AP_POLYGON)
    return failf(OL_EUNSUPPORTED, "surface %d: aperture kind %d", i, s.aperture_kind);
  if (s.coating_kind < OL_COAT_NONE || s.coating_kind > OL_COAT_RETARDER)
    return failf(OL_EUNSUPPORTED, "surface %d: coating kind %d", i, s.coating_kind);
  if (s.n_coeff < 0 || s.coeff_offset < 0)
    return failf(OL_EINVAL, "surface %d: negative coefficient range", i);
  if ((int64_t)s.coeff_offset + (int64_t)s.n_coeff * kind->per + kind->extra > n_coeffs)
    return failf(OL_EINVAL, "surface %d: coefficient block exceeds the buffer", i);
  return OL_OK;
}

// ---- common fields: kinds, flags, the base conic, the surface's own frame
inline void stage_common(const ol_surface_desc& s, const GeomKind& kind, HostSurf& d) {
  d.geom = kind.device;
  d.interaction = s.interaction;
  d.aperture_kind = s.aperture_kind;
  d.coating_kind = s.coating_kind;
  d.max_iter = s.max_iter;
  d.poly_cols = s.poly_cols;
  d.flags = (s.flags & OL_SURF_ROTATED) ? kSurfRotated : 0u;
  const bool inf_r = std::isinf(s.radius) || kind.flat;
  if (inf_r) d.flags |= kSurfRadiusInf;
  if ((s.flags & OL_SURF_REFERENCE_ROOT) && !inf_r && kind.reference_root)
    d.flags |= kSurfReferenceRoot;
  d.cv = inf_r ? 0.0 : 1.0 / s.radius;
  d.kp1 = 1.0 + s.conic;
  d.radius = s.radius;
  d.conic = s.conic;
  d.tol = s.tol;
  d.inv_norm = s.norm_radius != 0.0 ? 1.0 / s.norm_radius : 0.0;
  for (int k = 0; k < 3; ++k) d.origin[k] = s.origin[k];
  for (int k = 0; k < 9; ++k) d.rot[k] = s.rot[k];
  if (!(d.flags & kSurfRotated)) std::memcpy(d.rot, kIdentity3, sizeof(kIdentity3));
}

// ---- frame chain: the relative transform from the local frame of the previous TRACED surface `p`
// (the kernel keeps its state in that frame; record-only surfaces do not move it); NULL: none yet
inline void stage_frame(const HostSurf* p, HostSurf& d) {
  std::memcpy(d.rel_rot, kIdentity3, sizeof(kIdentity3));
  if (!p) return;
  mat3_mul_abt(d.rot, p->rot, d.rel_rot);
  double dv[3] = {p->origin[0] - d.origin[0], p->origin[1] - d.origin[1],
                  p->origin[2] - d.origin[2]};
  for (int r = 0; r < 3; ++r) {
    double v = d.rot[3 * r] * dv[0] + d.rot[3 * r + 1] * dv[1] + d.rot[3 * r + 2] * dv[2];
    d.rel_off[r] = std::isfinite(v) ? v : 0.0;
  }
  if (!is_identity(d.rel_rot)) d.flags |= kSurfRelRotated;
}

// ---- apertures: pre-square / pre-invert in double; polygon vertex blocks move into the device
// coefficient buffer and their token / descriptor offsets are rewritten
inline int stage_polygon(int32_t i, const StageIn& in, const double* a, double* q,
                         std::vector<double>& out) {
  const int64_t voff = (int64_t)a[0], nv = (int64_t)a[1];
  if (voff < 0 || nv < 1 || voff + 2 * nv > in.n_coeffs)
    return failf(OL_EINVAL, "surface %d: polygon vertex block outside the buffer", i);
  q[0] = (double)out.size();
  q[1] = (double)nv;
  q[2] = q[3] = 0.0;
  out.insert(out.end(), in.coeffs + voff, in.coeffs + voff + 2 * nv);
  return OL_OK;
}

inline int stage_aperture(int32_t i, const StageIn& in, const ol_surface_desc& s, HostSurf& d,
                          std::vector<double>& out) {
  if (s.aperture_kind == OL_AP_POLYGON) return stage_polygon(i, in, s.aperture, d.ap, out);
  if (s.aperture_kind != OL_AP_COMPOSITE) {
    convert_aperture(s.aperture_kind, s.aperture, d.ap);
    return OL_OK;
  }
  const int64_t off = (int64_t)s.aperture[0], cnt = (int64_t)s.aperture[1];
  if (off < 0 || cnt <= 0 || off + cnt * OL_AP_TOKEN_DOUBLES > in.n_coeffs)
    return failf(OL_EINVAL, "surface %d: aperture token list outside the buffer", i);
  // pass 1: converted tokens (polygon vertices are appended to `out` as they come)
  std::vector<double> toks;
  int depth = 0;
  for (int64_t t = 0; t < cnt; ++t) {
    const double* tok = in.coeffs + off + t * OL_AP_TOKEN_DOUBLES;
    const int op = (int)tok[0];
    double q[4];
    if (op >= OL_AP_RADIAL && op <= OL_AP_ELLIPTICAL) {
      convert_aperture(op, tok + 1, q);
      if (++depth > OL_AP_MAX_DEPTH)
        return failf(OL_EUNSUPPORTED, "surface %d: aperture tree too deep", i);
    } else if (op == OL_AP_POLYGON) {
      if (int rc = stage_polygon(i, in, tok + 1, q, out)) return rc;
      if (++depth > OL_AP_MAX_DEPTH)
        return failf(OL_EUNSUPPORTED, "surface %d: aperture tree too deep", i);
    } else if (op >= OL_AP_OP_UNION && op <= OL_AP_OP_DIFFERENCE) {
      q[0] = q[1] = q[2] = q[3] = 0.0;
      if (--depth < 1) return failf(OL_EINVAL, "surface %d: malformed aperture tokens", i);
    } else {
      return failf(OL_EUNSUPPORTED, "surface %d: aperture token op %d", i, op);
    }
    toks.push_back((double)op);
    toks.insert(toks.end(), q, q + 4);
  }
  if (depth != 1) return failf(OL_EINVAL, "surface %d: malformed aperture tokens", i);
  // pass 2: the token list itself, contiguous
  d.ap_off = (int32_t)out.size();
  d.ap_len = (int32_t)cnt;
  out.insert(out.end(), toks.begin(), toks.end());
  return OL_OK;
}

// ---- coating: the axis block of a polarizer (3 values) / retarder (+ the retardance)
inline int stage_coating(int32_t i, const StageIn& in, const ol_surface_desc& s, HostSurf& d) {
  d.coat[0] = s.coat[0];
  d.coat[1] = s.coat[1];
  if (s.coating_kind != OL_COAT_POLARIZER && s.coating_kind != OL_COAT_RETARDER) return OL_OK;
  const int need = s.coating_kind == OL_COAT_RETARDER ? 4 : 3;
  const int64_t off = (int64_t)s.coat[0];
  if (off < 0 || off + need > in.n_coeffs)
    return failf(OL_EINVAL, "surface %d: coating axis block outside the buffer", i);
  for (int k = 0; k < 3; ++k) d.axis[k] = in.coeffs[off + k];
  if (s.coating_kind == OL_COAT_RETARDER) {
    d.ret_cos = std::cos(in.coeffs[off + 3] / 2);
    d.ret_sin = std::sin(in.coeffs[off + 3] / 2);
  }
  return OL_OK;
}

// ---- coefficient blocks, one stager per family: public block -> device block, d.n_coeff
inline int stage_zernike(StageRow& r) {
  int ng = 0;
  if (zernike_mono_enabled() && build_zernike_mono_block(r.src, r.s.n_coeff, r.out, &ng))
    r.d.geom = kGeomZernikeMono;  // low order, well conditioned: one polynomial
  else if (build_zernike_block(r.src, r.s.n_coeff, r.out, r.int_slots, &ng) != 0)
    return failf(OL_EINVAL, "surface %d: invalid Zernike (n, m) index", r.i);
  r.d.n_coeff = ng;
  return OL_OK;
}

// even / odd aspheres and polynomials: the block as it is
inline int stage_copy(StageRow& r) {
  const ol_surface_desc& s = r.s;
  if (s.geom_kind == OL_GEOM_POLYNOMIAL && (s.poly_cols <= 0 || s.n_coeff % s.poly_cols != 0))
    return failf(OL_EINVAL, "surface %d: polynomial grid %d x ? cols %d", r.i, s.n_coeff,
                 s.poly_cols);
  r.d.n_coeff = s.n_coeff;
  r.out.insert(r.out.end(), r.src, r.src + s.n_coeff);
  return OL_OK;
}

inline int stage_chebyshev(StageRow& r) {
  const ol_surface_desc& s = r.s;
  if (s.poly_cols <= 0 || s.n_coeff % s.poly_cols != 0)
    return failf(OL_EINVAL, "surface %d: chebyshev grid %d, cols %d", r.i, s.n_coeff, s.poly_cols);
  r.d.n_coeff = s.n_coeff;
  r.out.push_back(1.0 / r.src[0]);
  r.out.push_back(1.0 / r.src[1]);
  r.out.insert(r.out.end(), r.src + 2, r.src + 2 + s.n_coeff);
  return OL_OK;
}

inline int stage_biconic(StageRow& r) {
  // biconic.py:57-66: cx/cy = 0 for infinite or zero radii
  if (r.s.n_coeff != 2) return failf(OL_EINVAL, "surface %d: biconic needs {Ry, ky}", r.i);
  const double Rx = r.s.radius, Ry = r.src[0];
  r.d.cv = (std::isinf(Rx) || Rx == 0.0) ? 0.0 : 1.0 / Rx;
  r.d.n_coeff = 2;
  r.out.push_back((std::isinf(Ry) || Ry == 0.0) ? 0.0 : 1.0 / Ry);
  r.out.push_back(1.0 + r.src[1]);
  return OL_OK;
}

inline int stage_toroidal(StageRow& r) {
  if (r.s.n_coeff < 2) return failf(OL_EINVAL, "surface %d: toroidal needs {R_rot, k_yz}", r.i);
  const double Rr = r.src[0], Ryz = r.s.radius;
  r.d.n_coeff = r.s.n_coeff - 2;  // number of y^(2i) terms
  r.out.push_back(Rr);
  r.out.push_back(std::isinf(Rr) ? 0.0 : 1.0 / Rr);
  r.out.push_back(1.0 + r.src[1]);
  r.out.push_back((std::isfinite(Ryz) && Ryz != 0.0) ? 1.0 / Ryz : 0.0);
  r.out.insert(r.out.end(), r.src + 2, r.src + r.s.n_coeff);
  return OL_OK;
}

// what both Forbes blocks are asked first
inline int check_forbes(const StageRow& r) {
  const ol_surface_desc& s = r.s;
  if (!(s.norm_radius > 0.0) || !std::isfinite(s.norm_radius))
    return failf(OL_EINVAL, "surface %d: Forbes norm_radius %g must be finite and positive", r.i,
                 s.norm_radius);
  if (s.interaction == OL_INTERACT_RECORD_ONLY)
    return failf(OL_EUNSUPPORTED, "surface %d: a Forbes surface that only records", r.i);
  for (int k = 0; k < s.n_coeff; ++k)
    if (!std::isfinite(r.src[k]))
      return failf(OL_EINVAL, "surface %d: Forbes coefficient block entry %d is not finite", r.i, k);
  return OL_OK;
}

// device block: n0, norm_radius, then the rest of the public block (forbes_device.h)
inline int stage_forbes_q(StageRow& r) {
  if (int rc = check_forbes(r)) return rc;
  r.d.n_coeff = r.s.n_coeff;
  r.int_slots.push_back(r.out.size());
  r.out.push_back((double)r.s.n_coeff);
  r.out.push_back(r.s.norm_radius);
  r.out.insert(r.out.end(), r.src, r.src + r.s.n_coeff);
  return OL_OK;
}

inline int stage_forbes_q2d(StageRow& r) {
  if (int rc = check_forbes(r)) return rc;
  const int64_t n = r.s.n_coeff;
  const double* src = r.src;
  r.d.n_coeff = r.s.n_coeff;
  // the block describes itself: walk it once, every count against what is left
  auto count_at = [&](int64_t at, int64_t& v) { return at < n && whole_count(src[at], n, v); };
  const size_t base = r.out.size();
  std::vector<size_t> ints;
  int64_t n0 = 0, M = 0, at = 2;
  bool ok = count_at(0, n0) && count_at(1, M) && at + n0 <= n;
  if (ok) {
    ints.push_back(0);           // n0        (device offsets: + 1 behind norm_radius)
    ints.push_back(2);           // M
    at += n0;
    for (int64_t mm = 0; ok && mm < M; ++mm) {
      int64_t na = 0, nb = 0;
      ok = count_at(at, na) && count_at(at + 1, nb) && at + 2 + 4 * (na + nb) <= n;
      if (ok) {
        ints.push_back((size_t)at + 1);
        ints.push_back((size_t)at + 2);
        at += 2 + 4 * (na + nb);
      }
    }
  }
  if (!ok || at != n)
    return failf(OL_EINVAL, "surface %d: Forbes Q2D block of %d values does not match the "
                            "counts it declares", r.i, r.s.n_coeff);
  r.out.push_back(src[0]);
  r.out.push_back(r.s.norm_radius);
  r.out.insert(r.out.end(), src + 1, src + n);
  for (size_t k : ints) r.int_slots.push_back(base + k);
  return OL_OK;
}

// public block {order, period, groove angle} -> device block (grating_device.h)
inline int stage_grating(StageRow& r) {
  const ol_surface_desc& s = r.s;
  const double* src = r.src;
  if (s.n_coeff != 3)
    return failf(OL_EINVAL, "surface %d: a grating needs {order, period, groove angle}", r.i);
  if (s.interaction == OL_INTERACT_RECORD_ONLY)
    return failf(OL_EUNSUPPORTED, "surface %d: a grating that only records", r.i);
  if (!std::isfinite(src[1]) || src[1] == 0.0)
    return failf(OL_EINVAL, "surface %d: grating period %g must be finite and not zero", r.i,
                 src[1]);
  if (!std::isfinite(src[0]) || !std::isfinite(src[2]))
    return failf(OL_EINVAL, "surface %d: grating order %g / groove angle %g must be finite", r.i,
                 src[0], src[2]);
  if (s.geom_kind == OL_GEOM_STANDARD_GRATING &&
      ((r.d.flags & kSurfRadiusInf) || !(s.radius != 0.0)))
    return failf(OL_EINVAL, "surface %d: a standard grating needs a finite radius that is not "
                            "zero (a flat one is OL_GEOM_PLANE_GRATING)", r.i);
  r.d.n_coeff = 3;
  r.out.push_back(src[0]);
  r.out.push_back(src[1]);
  r.out.push_back(std::sin(src[2]));
  r.out.push_back(std::cos(src[2]));
  r.out.push_back(std::tan(src[2]));
  return OL_OK;
}

// The self-describing block of an OL_GEOM_PLANE_PHASE row (ol_geom_kind in optiland_hip.h), checked
// value by value and appended in the layout phase_device.h reads.
inline int stage_phase(StageRow& r, int32_t n_wl) {
  const int32_t i = r.i;
  const double* src = r.src;
  std::vector<double>& out = r.out;
  const int64_t n = r.s.n_coeff;
  if (r.s.interaction == OL_INTERACT_RECORD_ONLY)
    return failf(OL_EUNSUPPORTED, "surface %d: a phase surface that only records", i);
  int64_t kind = 0;
  if (n < 2 || !whole_count(src[0], n, kind) || kind > 3)
    return failf(OL_EINVAL, "surface %d: phase profile kind %g is not 0 (constant), 1 (linear), "
                            "2 (radial) or 3 (grid)", i, n >= 1 ? src[0] : -1.0);
  if (!std::isfinite(src[1]))
    return failf(OL_EINVAL, "surface %d: phase profile efficiency %g must be finite", i, src[1]);
  r.d.n_coeff = r.s.n_coeff;
  const size_t base = out.size();
  r.int_slots.push_back(base);
  if (kind == kPhaseConstant || kind == kPhaseLinear) {
    const int64_t need = kind == kPhaseConstant ? 3 : 4;
    if (n != need)
      return failf(OL_EINVAL, "surface %d: a %s phase block holds %lld values, not %lld", i,
                   kind == kPhaseConstant ? "constant" : "linear", (long long)need,
                   (long long)n);
    out.insert(out.end(), src, src + n);
    return OL_OK;
  }
  if (kind == kPhaseRadial) {
    int64_t count = 0;
    if (n < 3 || !whole_count(src[2], n, count) || 3 + count != n)
      return failf(OL_EINVAL, "surface %d: radial phase block of %lld values does not match the "
                              "term count %g it declares", i, (long long)n, n >= 3 ? src[2] : -1.0);
    r.int_slots.push_back(base + 2);
    out.insert(out.end(), src, src + n);
    return OL_OK;
  }
  int64_t W = 0, H = 0, n_scale = 0;
  if (n < 9 || !whole_count(src[2], n, W) || !whole_count(src[3], n, H) || W < 2 || H < 2)
    return failf(OL_EINVAL, "surface %d: a phase grid needs whole node counts W, H >= 2 (got %g, "
                            "%g)", i, n >= 9 ? src[2] : -1.0, n >= 9 ? src[3] : -1.0);
  for (int k = 4; k < 8; ++k)
    if (!std::isfinite(src[k]))
      return failf(OL_EINVAL, "surface %d: phase grid bound %g is not finite", i, src[k]);
  if (src[5] == src[4] || src[7] == src[6])
    return failf(OL_EINVAL, "surface %d: phase grid bounds coincide (x %g .. %g, y %g .. %g)", i,
                 src[4], src[5], src[6], src[7]);
  if (!whole_count(src[8], n, n_scale) || (n_scale != 0 && n_scale != n_wl))
    return failf(OL_EINVAL, "surface %d: phase grid scale count %g is neither 0 nor the "
                            "wavelength count %d", i, src[8], n_wl);
  if (9 + n_scale + W * H != n)
    return failf(OL_EINVAL, "surface %d: phase grid block of %lld values does not match the "
                            "counts it declares (9 + %lld scales + %lld x %lld nodes)", i,
                 (long long)n, (long long)n_scale, (long long)W, (long long)H);
  const double xs = src[5] - src[4], ys = src[7] - src[6];
  const double head[kPhaseGridHead] = {
      src[0], src[1], (double)W, (double)H, src[4], xs, src[6], ys, (double)(W - 1),
      (double)(H - 1), (double)(W - 1) / xs, (double)(H - 1) / ys, (double)n_scale};
  out.insert(out.end(), head, head + kPhaseGridHead);
  r.int_slots.push_back(base + 2);
  r.int_slots.push_back(base + 3);
  r.int_slots.push_back(base + 12);
  out.insert(out.end(), src + 9, src + n);
  return OL_OK;
}

// The self-describing block of an OL_GEOM_GRID_SAG row (ol_geom_kind in optiland_hip.h), checked
// value by value and appended in the layout grid_sag_device.h reads.
inline int stage_grid_sag(StageRow& r) {
  const int32_t i = r.i;
  const double* src = r.src;
  std::vector<double>& out = r.out;
  const int64_t n = r.s.n_coeff;
  if (r.s.interaction == OL_INTERACT_RECORD_ONLY)
    return failf(OL_EUNSUPPORTED, "surface %d: a grid-sag surface that only records", i);
  int64_t W = 0, H = 0;
  if (n < 2 || !whole_count(src[0], n, W) || !whole_count(src[1], n, H) || W < 2 || H < 2)
    return failf(OL_EINVAL, "surface %d: a sag grid needs whole node counts W, H >= 2 (got %g, "
                            "%g)", i, n >= 2 ? src[0] : -1.0, n >= 2 ? src[1] : -1.0);
  // (the last cell, W - 2, is a float in the fp32 table: exact up to 2^24)
  if (W > (1 << 24) || H > (1 << 24))
    return failf(OL_EINVAL, "surface %d: a sag grid takes at most 16777216 nodes on an axis (got "
                            "%lld, %lld)", i, (long long)W, (long long)H);
  if (2 + W + H + W * H != n)
    return failf(OL_EINVAL, "surface %d: sag grid block of %lld values does not match the counts "
                            "it declares (2 + %lld + %lld coordinates + %lld x %lld nodes)", i,
                 (long long)n, (long long)W, (long long)H, (long long)W, (long long)H);
  for (int64_t k = 2; k < n; ++k)
    if (!std::isfinite(src[k]))
      return failf(OL_EINVAL, "surface %d: sag grid value %lld (%g) is not finite", i,
                   (long long)k, src[k]);
  const double* xs = src + 2;
  const double* ys = xs + W;
  auto increasing = [&](const double* v, int64_t cnt, const char* axis) {
    for (int64_t k = 1; k < cnt; ++k)
      if (!(v[k] > v[k - 1]) || !((float)v[k] > (float)v[k - 1]))
        return failf(OL_EINVAL, "surface %d: sag grid %s coordinates are not strictly increasing "
                                "(as doubles and as floats) at index %lld: %.17g, %.17g", i, axis,
                     (long long)k, v[k - 1], v[k]);
    return (int)OL_OK;
  };
  if (int rc = increasing(xs, W, "x")) return rc;
  if (int rc = increasing(ys, H, "y")) return rc;
  r.d.n_coeff = r.s.n_coeff;
  const size_t base = out.size();
  const double head[kGridSagHead] = {
      (double)W, (double)H, (double)(W - 2), (double)(H - 2), xs[0], xs[W - 1], ys[0], ys[H - 1],
      (double)(W - 1) / (xs[W - 1] - xs[0]), (double)(H - 1) / (ys[H - 1] - ys[0])};
  out.insert(out.end(), head, head + kGridSagHead);
  r.int_slots.push_back(base);
  r.int_slots.push_back(base + 1);
  out.insert(out.end(), src + 2, src + n);
  return OL_OK;
}

inline int stage_block(StageRow& r, int32_t n_wl) {
  switch (r.s.geom_kind) {
    case OL_GEOM_ZERNIKE: return stage_zernike(r);
    case OL_GEOM_EVEN_ASPHERE:
    case OL_GEOM_ODD_ASPHERE:
    case OL_GEOM_POLYNOMIAL: return stage_copy(r);
    case OL_GEOM_CHEBYSHEV: return stage_chebyshev(r);
    case OL_GEOM_BICONIC: return stage_biconic(r);
    case OL_GEOM_TOROIDAL: return stage_toroidal(r);
    case OL_GEOM_FORBES_Q: return stage_forbes_q(r);
    case OL_GEOM_FORBES_Q2D: return stage_forbes_q2d(r);
    case OL_GEOM_PLANE_GRATING:
    case OL_GEOM_STANDARD_GRATING: return stage_grating(r);
    case OL_GEOM_PLANE_PHASE: return stage_phase(r, n_wl);
    case OL_GEOM_GRID_SAG: return stage_grid_sag(r);
    default: r.d.n_coeff = 0; return OL_OK;   // a plane, a conic: no block
  }
}

// ---- what the entry points validate against (HostFacts), from an accepted table
inline void stage_facts(const StageIn& in, int32_t n_surf, const std::vector<HostSurf>& dev,
                        HostFacts& f) {
  for (int32_t i = 0; i < n_surf; ++i) {
    const ol_surface_desc& s = in.surf[i];
    f.interaction.push_back(s.interaction);
    f.coating.push_back(s.coating_kind);
    f.geom.push_back(s.geom_kind);
    bool poly = s.aperture_kind == OL_AP_POLYGON;
    if (s.aperture_kind == OL_AP_COMPOSITE) {
      const int64_t off = (int64_t)s.aperture[0], cnt = (int64_t)s.aperture[1];
      for (int64_t t = 0; t < cnt; ++t)
        poly = poly || (int)in.coeffs[off + t * OL_AP_TOKEN_DOUBLES] == OL_AP_POLYGON;
    }
    f.polygon.push_back(poly ? 1 : 0);
    f.no_pair.push_back((s.geom_kind == OL_GEOM_ZERNIKE && dev[i].geom != kGeomZernikeMono) ||
                                s.coating_kind == OL_COAT_POLARIZER ||
                                s.coating_kind == OL_COAT_RETARDER
                            ? 1 : 0);
    f.ref_newton.push_back((s.flags & OL_SURF_REFERENCE_NEWTON) && geom_kind(s.geom_kind)->newton &&
                                   s.interaction != OL_INTERACT_RECORD_ONLY
                               ? 1 : 0);
  }
}

// Which Newton kernel a traced range needs (trace_launch.h: launch_trace): 0 = none,
// 3 / 4 = all of its Newton-Raphson surfaces are Zernike surfaces / even aspheres, 5 = the
// reference's batch-global stop rule was asked for (OL_SURF_REFERENCE_NEWTON), else 1.
// (A polygon aperture on a conic-only range also selects the generic kernel: polygons live
// in the full kernels only.)
inline int newton_family_of(const HostFacts& f, int32_t first, int32_t last) {
  bool any = false, polygon = false, all_zernike = true, all_even = true;
  // OL_SURF_REFERENCE_NEWTON (opt-in, ABI 11) on any Newton surface of the range: the kernel
  // family that iterates the batch in lockstep (surface_math.h: newton_reference)
  for (int32_t s = first; s <= last; ++s)
    if (f.ref_newton[s]) return kNrReference;
  for (int32_t s = first; s <= last; ++s) {
    polygon = polygon || f.polygon[s];
    const int g = f.geom[s];
    if (g == OL_GEOM_PLANE || g == OL_GEOM_STANDARD) continue;
    any = true;
    all_zernike = all_zernike && g == OL_GEOM_ZERNIKE;
    all_even = all_even && g == OL_GEOM_EVEN_ASPHERE;
  }
  if (!any) return polygon ? 1 : 0;
  // OPTILAND_HIP_NR_FAMILY=0: always the generic Newton kernel (A/B runs; parity tests of the
  // generic instantiation on single-family systems)
  static const bool families = [] {
    const char* e = getenv("OPTILAND_HIP_NR_FAMILY");
    return !(e && e[0] == '0');
  }();
  if (families && all_zernike) return 3;
  if (families && all_even) return 4;
  return 1;
}

// argument validation + every host-side conversion of ol_system_create / ol_system_update
inline int stage_system(const char* who, const ol_surface_desc* surf, int32_t n_surf,
                        const double* coeffs, int32_t n_coeffs, const ol_surface_optics* optics,
                        int32_t n_wavelengths, Staged& st) {
  if (!surf || n_surf <= 0) return failf(OL_EINVAL, "%s: no surfaces", who);
  if (!optics || n_wavelengths <= 0) return failf(OL_EINVAL, "%s: no optics table", who);
  if (n_coeffs < 0 || (n_coeffs > 0 && !coeffs))
    return failf(OL_EINVAL, "%s: bad coefficient buffer", who);
  const StageIn in{surf, coeffs, n_coeffs};

  st.surf.assign(n_surf, HostSurf());
  const HostSurf* prev_traced = nullptr;
  for (int32_t i = 0; i < n_surf; ++i) {
    const ol_surface_desc& s = surf[i];
    HostSurf& d = st.surf[i];
    std::memset(&d, 0, sizeof(d));
    const GeomKind* kind = nullptr;
    if (int rc = check_row(i, s, n_coeffs, kind)) return rc;
    stage_common(s, *kind, d);
    stage_frame(prev_traced, d);
    if (s.interaction != OL_INTERACT_RECORD_ONLY) prev_traced = &d;
    if (int rc = stage_aperture(i, in, s, d, st.coeffs)) return rc;
    if (int rc = stage_coating(i, in, s, d)) return rc;
    d.coeff_off = (int32_t)st.coeffs.size();
    StageRow row{i, s, d, coeffs ? coeffs + s.coeff_offset : nullptr, st.coeffs, st.int_slots};
    if (int rc = stage_block(row, n_wavelengths)) return rc;
    d.coeff_len = (int32_t)st.coeffs.size() - d.coeff_off;
  }

  st.optics.assign((size_t)n_surf * n_wavelengths, DevOptics<double>());
  for (size_t i = 0; i < st.optics.size(); ++i) {
    const ol_surface_optics& o = optics[i];
    DevOptics<double>& d = st.optics[i];
    std::memset(&d, 0, sizeof(d));
    d.n1 = o.n1;
    d.n2 = o.n2;
    d.u = o.n1 / o.n2;
    d.nn = o.n2 / o.n1;
    d.absorb = o.absorb > 0.0 ? o.absorb : 0.0;
  }
  stage_facts(in, n_surf, st.surf, st.facts);
  return OL_OK;
}

}  // namespace ol
