// table_image.h -- a staged table (system_stage.h: HostSurf rows, optics rows and coefficients,
// all in double) written out as the rows the kernels read (device_table.h) in the working
// precision T.  Host-only, no HIP runtime: the one conversion behind every upload -- the single
// table of an ol_system (capi.hip) and the stacked tables of an ol_ensemble (ensemble.hip).
#pragma once
#include <stdint.h>

#include <cstring>
#include <type_traits>
#include <vector>

#include "device_table.h"
#include "system_stage.h"

namespace ol {

// `surf` / `cold`: surf64.size() rows each, `opt`: opt64.size() rows, `coef`: coef64.size() values
template <typename T>
inline void write_table_image(const std::vector<HostSurf>& surf64,
                              const std::vector<DevOptics<double>>& opt64,
                              const std::vector<double>& coef64,
                              const std::vector<size_t>& int_slots, DevSurfHot<T>* surf,
                              DevSurfCold<T>* cold, DevOptics<T>* opt, T* coef) {
  for (size_t i = 0; i < surf64.size(); ++i) {
    const HostSurf& a = surf64[i];
    DevSurfHot<T>& b = surf[i];
    DevSurfCold<T>& c = cold[i];
    b.geom = a.geom; b.interaction = a.interaction; b.aperture_kind = a.aperture_kind;
    b.coating_kind = a.coating_kind; b.coeff_off = a.coeff_off; b.n_coeff = a.n_coeff;
    b.max_iter = a.max_iter; b.flags = a.flags;
    b.cv = (T)a.cv; b.kp1 = (T)a.kp1;
    c.poly_cols = a.poly_cols; c.coeff_len = a.coeff_len; c.ap_off = a.ap_off;
    c.ap_len = a.ap_len; c.tol = (T)a.tol; c.inv_norm = (T)a.inv_norm;
    for (int k = 0; k < 3; ++k) { b.origin[k] = (T)a.origin[k]; b.rel_off[k] = (T)a.rel_off[k]; }
    for (int k = 0; k < 9; ++k) { c.rot[k] = (T)a.rot[k]; c.rel_rot[k] = (T)a.rel_rot[k]; }
    for (int k = 0; k < 4; ++k) c.ap[k] = (T)a.ap[k];
    for (int k = 0; k < 2; ++k) c.coat[k] = (T)a.coat[k];
    for (int k = 0; k < 3; ++k) c.axis[k] = (T)a.axis[k];
    c.ret_cos = (T)a.ret_cos; c.ret_sin = (T)a.ret_sin;
    c.radius = (T)a.radius; c.conic = (T)a.conic;
  }
  for (size_t i = 0; i < opt64.size(); ++i) {
    opt[i].n1 = (T)opt64[i].n1; opt[i].n2 = (T)opt64[i].n2; opt[i].u = (T)opt64[i].u;
    opt[i].nn = (T)opt64[i].nn; opt[i].absorb = (T)opt64[i].absorb;
  }
  for (size_t i = 0; i < coef64.size(); ++i) coef[i] = (T)coef64[i];
  for (size_t i : int_slots) {  // loop headers: integer bit patterns (scalar-unit operands)
    using I = typename std::conditional<sizeof(T) == 4, int32_t, int64_t>::type;
    const I v = (I)coef64[i];
    std::memcpy(&coef[i], &v, sizeof(T));
  }
}

}  // namespace ol
