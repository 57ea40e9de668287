// capi.hip -- the C ABI declared in include/optiland_hip.h.
//
// Host-side only: validates arguments, uploads the staged surface table as
// DevSurf<T>/DevOptics<T> for T in {float, double} (device_table.h) and launches
// the kernels on the caller's stream.  No ray memory is ever allocated here.
// Staging -- the public table re-expressed in double, and everything it refuses -- is
// system_stage.h (with zernike_stage.h and the kind table geom_kinds.h), host-only headers.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/optiland_hip.h"
#include "device_table.h"
#include "entry_rules.h"
#include "last_error.h"
#include "system_stage.h"
#include "system_view.h"
#include "table_image.h"
#include "trace_launch.h"

namespace {
thread_local std::string g_err;
}

int ol::failf(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

namespace {

using namespace ol;   // failf and the shared argument rules (entry_rules.h)

#define OL_HIP_CHECK(expr)                                                        \
  do {                                                                            \
    hipError_t e_ = (expr);                                                       \
    if (e_ != hipSuccess)                                                         \
      return failf(OL_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_));        \
  } while (0)

template <typename T>
struct DeviceTable {
  // ONE allocation: [hot rows | cold rows | optics rows | coefficients], each block on a
  // 256-byte boundary -- created by one copy and re-written in place by one copy
  // (ol_system_update: an optimiser edits the prescription between every two traces)
  char* blob = nullptr;
  ol::DevSurfHot<T>* surf = nullptr;
  ol::DevSurfCold<T>* cold = nullptr;
  ol::DevOptics<T>* optics = nullptr;
  T* coeffs = nullptr;
  size_t n_surf = 0, n_opt = 0, coef_capacity = 0;  // allocation sizes (ol_system_update)
  size_t off_cold = 0, off_opt = 0, off_coef = 0;
};

inline size_t round256(size_t v) { return (v + 255u) & ~size_t(255u); }

}  // namespace

struct ol_system {
  int32_t n_surf = 0;
  int32_t n_wl = 0;
  int device = 0;
  DeviceTable<float> f32;
  DeviceTable<double> f64;
  HostFacts facts;   // host copies for validation (system_stage.h)
  // false between the two in-place uploads of ol_system_update and for good if the second
  // one fails: the fp32 and fp64 tables (and the host copies) then describe different
  // prescriptions -- every entry point refuses such a system instead of tracing through it
  bool consistent = true;
};

namespace {

// in_place: the allocation of `dst` is reused (it must fit: checked by the caller) and the
// copy is queued on `stream`, i.e. ordered after every launch already queued there that
// still reads the old table; otherwise a fresh allocation and a blocking copy.
template <typename T>
int upload(const std::vector<HostSurf>& surf64,
           const std::vector<ol::DevOptics<double>>& opt64, const std::vector<double>& coef64,
           const std::vector<size_t>& int_slots, DeviceTable<T>& dst, bool in_place = false,
           hipStream_t stream = nullptr) {
  const size_t n_surf = surf64.size(), n_opt = opt64.size();
  const size_t n_coef = coef64.size() ? coef64.size() : 1;
  const size_t off_cold = round256(n_surf * sizeof(ol::DevSurfHot<T>));
  const size_t off_opt = off_cold + round256(n_surf * sizeof(ol::DevSurfCold<T>));
  const size_t off_coef = off_opt + round256(n_opt * sizeof(ol::DevOptics<T>));
  const size_t used = off_coef + n_coef * sizeof(T);
  std::vector<char> host(used, 0);
  auto* surf = reinterpret_cast<ol::DevSurfHot<T>*>(host.data());
  auto* cold = reinterpret_cast<ol::DevSurfCold<T>*>(host.data() + off_cold);
  auto* opt = reinterpret_cast<ol::DevOptics<T>*>(host.data() + off_opt);
  T* coef = reinterpret_cast<T*>(host.data() + off_coef);
  ol::write_table_image<T>(surf64, opt64, coef64, int_slots, surf, cold, opt, coef);

  if (in_place) {
    // same surface / wavelength counts (checked by the caller): the block offsets are the
    // ones of the allocation.  (Pageable source: the runtime stages it before it returns,
    // the vector may go.)
    OL_HIP_CHECK(hipMemcpyAsync(dst.blob, host.data(), used, hipMemcpyHostToDevice, stream));
    return OL_OK;
  }
  dst.n_surf = n_surf;
  dst.n_opt = n_opt;
  // head room: a surface whose coefficient block grows a little (an asphere gaining a term)
  // still updates in place
  dst.coef_capacity = n_coef + 64;
  dst.off_cold = off_cold; dst.off_opt = off_opt; dst.off_coef = off_coef;
  OL_HIP_CHECK(hipMalloc((void**)&dst.blob, off_coef + dst.coef_capacity * sizeof(T)));
  dst.surf = reinterpret_cast<ol::DevSurfHot<T>*>(dst.blob);
  dst.cold = reinterpret_cast<ol::DevSurfCold<T>*>(dst.blob + off_cold);
  dst.optics = reinterpret_cast<ol::DevOptics<T>*>(dst.blob + off_opt);
  dst.coeffs = reinterpret_cast<T*>(dst.blob + off_coef);
  OL_HIP_CHECK(hipMemcpy(dst.blob, host.data(), used, hipMemcpyHostToDevice));
  return OL_OK;
}

template <typename T>
void release(DeviceTable<T>& t) {
  if (t.blob) (void)hipFree(t.blob);
  t = DeviceTable<T>();
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the Newton kernel family of a traced range (system_stage.h: newton_family_of)
int newton_family(const ol_system* sys, int32_t first, int32_t last) {
  return newton_family_of(sys->facts, first, last);
}

template <typename T>
int do_trace(const ol_system* sys, const DeviceTable<T>& tab, int64_t n, void* const rays[8],
             int32_t wl, void* record, int64_t record_stride, void* prt, int32_t first,
             int32_t last, uint32_t flags, uint32_t* status, const ol_trace_extras* extras,
             hipStream_t stream) {
  ol::TraceArgs<T> a{};
  a.spot = extras ? extras->spot_slots : nullptr;
  a.cx = extras ? extras->cx : 0.0;
  a.cy = extras ? extras->cy : 0.0;
  a.spot_slots = OL_SPOT_SLOTS;
  a.surf = tab.surf;
  a.cold = tab.cold;
  a.optics = tab.optics;
  a.coeffs = tab.coeffs;
  bool vec = true;
  constexpr int64_t kVec = 16 / sizeof(T);
  for (int k = 0; k < 8; ++k) {
    a.rays[k] = static_cast<T*>(rays[k]);
    vec = vec && aligned16(rays[k]);
  }
  a.record = static_cast<T*>(record);
  a.prt = static_cast<T*>(prt);
  if (record) vec = vec && aligned16(record) && (record_stride % kVec == 0);
  if (prt) vec = vec && aligned16(prt) && (n % kVec == 0);
  a.status = status;
  a.n = n;
  a.record_stride = record_stride;
  a.first = first;
  a.last = last;
  a.n_wl = sys->n_wl;
  a.wl = wl;
  a.flags = flags & 0xffu;  // public flags only
  a.record_from = (extras && extras->record_first_surface > first) ? extras->record_first_surface
                                                                     : first;
  if (!prt) a.flags &= ~ol::kTracePrtIdentity;
  // Zero-copy object row: when the caller's ray planes ARE row 0 of the record
  // block and the first surface only records (ObjectSurface.trace,
  // surfaces/object_surface.py:56-69), the kernel skips that row's stores.
  if (record && a.record_from == first && sys->facts.interaction[first] == OL_INTERACT_RECORD_ONLY) {
    bool alias = true;
    for (int k = 0; k < 8; ++k)
      alias = alias && (static_cast<T*>(rays[k]) == static_cast<T*>(record) + k * record_stride);
    if (alias) a.flags |= ol::kTraceRow0IsInput;
  }
  const int family = newton_family(sys, first, last);
  a.nr_iters = extras ? extras->newton_iterations : nullptr;
  a.nr_count_at = extras && extras->newton_iterations ? extras->newton_count_surface : -1;
  a.n_surf = sys->n_surf;
  if (family == ol::kNrReference) {
    if (!a.nr_iters)
      return failf(OL_EINVAL, "ol_trace: a surface of the range carries OL_SURF_REFERENCE_NEWTON: "
                              "pass ol_trace_extras.newton_iterations (see ol_newton_count)");
    if (a.spot)
      return failf(OL_EUNSUPPORTED, "ol_trace_ex: no spot epilogue on a reference-Newton range");
  }
  hipError_t e = ol::launch_trace<T>(a, vec, family, stream);
  if (e != hipSuccess) return failf(OL_EHIP, "trace launch failed: %s", hipGetErrorString(e));
  return OL_OK;
}

// ol_raygen_inputs -> working precision; host-side part of the range validation
// (launch-uniform scalars are checked here, planes in the kernel)
template <typename T>
int convert_inputs(const char* who, const ol_raygen_inputs* in, uint32_t* status,
                   ol::RaygenIn<T>& o, bool& aligned) {
  if (!in || !in->px || !in->py) return failf(OL_EINVAL, "%s: NULL argument", who);
  if ((in->hx == nullptr) != (in->hy == nullptr) || (in->vx == nullptr) != (in->vy == nullptr))
    return failf(OL_EINVAL, "%s: hx/hy (and vx/vy) must be given together", who);
  if ((in->flags & (OL_RAYGEN_CHECK_FIELD | OL_RAYGEN_CHECK_PUPIL)) && !status)
    return failf(OL_EINVAL, "%s: a CHECK flag needs a status word", who);
  if ((in->flags & OL_RAYGEN_CHECK_FIELD) && !in->hx) {
    auto bad = [](double v) { return !(v >= -1.0 && v <= 1.0); };
    if (bad(in->hx0) || bad(in->hy0))  // real_ray_tracer.py:156-173, same text
      return failf(OL_EINVAL, "Normalized field coordinates must be within (-1, 1)");
  }
  o.hx = static_cast<const T*>(in->hx);
  o.hy = static_cast<const T*>(in->hy);
  o.px = static_cast<const T*>(in->px);
  o.py = static_cast<const T*>(in->py);
  o.vx = static_cast<const T*>(in->vx);
  o.vy = static_cast<const T*>(in->vy);
  o.hx0 = (T)in->hx0;
  o.hy0 = (T)in->hy0;
  o.vx0 = (T)in->vx0;
  o.vy0 = (T)in->vy0;
  o.tx0 = o.ty0 = T(0);
  o.flags = in->flags;
  aligned = aligned16(in->px) && aligned16(in->py) && aligned16(in->hx) && aligned16(in->hy) &&
            aligned16(in->vx) && aligned16(in->vy);  // NULL counts as aligned
  return OL_OK;
}

ol::RaygenDev raygen_dev(const ol_raygen_params* g) {
  return ol::RaygenDev{g->object_infinite, g->field_kind, g->EPL,     g->EPD,    g->max_field,
                       g->offset,          g->z_first,    g->tele_dz, g->apod_a, g->apod_b,
                       g->apod_kind};
}

template <typename T>
int do_generate_rays(const ol_raygen_params* p, int64_t n, const ol_raygen_inputs* in,
                     void* const out[8], uint32_t* status, hipStream_t stream) {
  ol::RaygenIn<T> ri;
  bool al = true;
  if (int rc = convert_inputs<T>("ol_generate_rays", in, status, ri, al)) return rc;
  if (n == 0) return OL_OK;
  T* o[8];
  for (int k = 0; k < 8; ++k) o[k] = static_cast<T*>(out[k]);
  hipError_t e = ol::launch_raygen<T>(raygen_dev(p), ri, n, o, status, stream);
  if (e != hipSuccess) return failf(OL_EHIP, "raygen launch failed: %s", hipGetErrorString(e));
  return OL_OK;
}

template <typename T>
int do_trace_generate(const ol_system* sys, const DeviceTable<T>& tab, int64_t n,
                      const ol_raygen_params* p, const ol_raygen_inputs* in, int32_t wl,
                      void* record, int64_t record_stride, void* const rays_out[8], void* prt,
                      uint32_t flags, uint32_t* status, const ol_trace_extras* extras,
                      hipStream_t stream) {
  ol::TraceArgs<T> a{};
  bool al = true;
  if (int rc = convert_inputs<T>("ol_trace_generate", in, status, a.in, al)) return rc;
  if (n == 0) return OL_OK;
  a.spot = extras ? extras->spot_slots : nullptr;
  a.cx = extras ? extras->cx : 0.0;
  a.cy = extras ? extras->cy : 0.0;
  a.spot_slots = OL_SPOT_SLOTS;
  a.surf = tab.surf;
  a.cold = tab.cold;
  a.optics = tab.optics;
  a.coeffs = tab.coeffs;
  const ol::RaygenDev rg = raygen_dev(p);
  a.rgc = ol::RaygenConsts<T>(rg);
  if (a.in.hx == nullptr) ol::uniform_field_tangents<T>(rg, a.in);
  for (int k = 0; k < 8; ++k) a.rays[k] = rays_out ? static_cast<T*>(rays_out[k]) : nullptr;
  a.record = static_cast<T*>(record);
  a.prt = static_cast<T*>(prt);
  a.status = status;
  a.n = n;
  a.record_stride = record_stride;
  a.first = 0;
  a.last = sys->n_surf - 1;
  a.record_from = (extras && extras->record_first_surface > 0) ? extras->record_first_surface : 0;
  a.n_wl = sys->n_wl;
  a.wl = wl;
  a.flags = (flags & (ol::kTracePrtComplex | ol::kTraceFewWaves)) |
            (prt ? ol::kTracePrtIdentity : 0u) | (rays_out ? ol::kTraceWriteRays : 0u);
  if (extras && extras->updated_intensity && extras->update_intensity_state) {
    if (!prt)
      return failf(OL_EINVAL, "ol_trace_generate: the update_intensity epilogue needs a "
                              "polarised launch (prt)");
    const ol_polarization_state* ps = extras->update_intensity_state;
    ol::PolStateDev st{ps->is_polarized, ps->Ex, ps->Ey, ps->phase_x, ps->phase_y};
    a.pf = ol::PolFields<T>(st);
    a.i_updated = static_cast<T*>(extras->updated_intensity);
  }
  // packed pairs (fp32 lean form): 8-byte accesses to px / py, the record rows, the final state
  bool pair_ok = al && (reinterpret_cast<uintptr_t>(record) % 8 == 0) && record_stride % 2 == 0;
  if (rays_out)
    for (int k = 0; k < 8; ++k)
      pair_ok = pair_ok && reinterpret_cast<uintptr_t>(rays_out[k]) % 8 == 0;
  const int family = newton_family(sys, 0, sys->n_surf - 1);
  if (family == ol::kNrZernike) {
    // the polarised Zernike pair (fp32): polynomial-form Zernike surfaces, real diagonal Jones
    // matrices, an even number of rays (the PRT planes are written with 8-byte lane accesses)
    for (int32_t s = 0; s < sys->n_surf; ++s) pair_ok = pair_ok && !sys->facts.no_pair[s];
    pair_ok = pair_ok && prt && n % 2 == 0 && reinterpret_cast<uintptr_t>(prt) % 8 == 0 &&
              reinterpret_cast<uintptr_t>(a.i_updated) % 8 == 0;
  }
  hipError_t e = ol::launch_trace_generate<T>(a, family, pair_ok, stream);
  if (e != hipSuccess) return failf(OL_EHIP, "trace launch failed: %s", hipGetErrorString(e));
  return OL_OK;
}

template <typename T>
int do_trace_spot(const ol_system* sys, const DeviceTable<T>& tab, int64_t n,
                  const ol_raygen_params* p, const ol_raygen_inputs* in, double cx, double cy,
                  int32_t wl, void* const hits[3], double* out7, uint32_t* status,
                  hipStream_t stream) {
  ol::SpotArgs<T> a{};
  bool vec = true;
  if (int rc = convert_inputs<T>("ol_trace_spot", in, status, a.in, vec)) return rc;
  if (n == 0) return OL_OK;
  a.surf = tab.surf;
  a.cold = tab.cold;
  a.optics = tab.optics;
  a.coeffs = tab.coeffs;
  a.rg = raygen_dev(p);
  a.cx = cx;
  a.cy = cy;
  for (int k = 0; k < 3; ++k) {
    a.hits[k] = hits ? static_cast<T*>(hits[k]) : nullptr;
    vec = vec && aligned16(a.hits[k]);
  }
  a.out = out7;
  a.status = status;
  a.n = n;
  a.first = 0;
  a.last = sys->n_surf - 1;
  a.n_wl = sys->n_wl;
  a.wl = wl;
  a.tiles_per_block = 1;
  hipError_t e = ol::launch_spot_trace<T>(a, vec, newton_family(sys, 0, sys->n_surf - 1), stream);
  if (e != hipSuccess) return failf(OL_EHIP, "spot launch failed: %s", hipGetErrorString(e));
  return OL_OK;
}

template <typename T>
const DeviceTable<T>& table_of(const ol_system* sys);
template <>
const DeviceTable<float>& table_of<float>(const ol_system* sys) { return sys->f32; }
template <>
const DeviceTable<double>& table_of<double>(const ol_system* sys) { return sys->f64; }

// f(T(0)) for the working type T of `dt` (OL_F32: float, else double: the entry has checked it);
// with a system, f(T(0), the system's table of that precision)
template <typename F>
auto by_dtype(ol_dtype dt, F&& f) {
  return dt == OL_F32 ? f(float(0)) : f(double(0));
}
template <typename F>
int by_dtype(ol_dtype dt, const ol_system* sys, F&& f) {
  return dt == OL_F32 ? f(float(0), sys->f32) : f(double(0), sys->f64);
}

template <typename T>
int do_trace_spot_batch(const ol_system* sys, const DeviceTable<T>& tab, int64_t n,
                        const ol_raygen_params* p, const ol_raygen_inputs* in, int32_t n_cells,
                        const ol_spot_cell* cells, void* hits, int64_t hits_stride, double* out8,
                        uint32_t* status, hipStream_t stream) {
  ol::SpotArgs<T> a{};
  bool vec = true;
  if (int rc = convert_inputs<T>("ol_trace_spot_batch", in, status, a.in, vec)) return rc;
  if (n == 0 || n_cells == 0) return OL_OK;
  a.surf = tab.surf;
  a.cold = tab.cold;
  a.optics = tab.optics;
  a.coeffs = tab.coeffs;
  a.rg = raygen_dev(p);
  T* hb = static_cast<T*>(hits);
  for (int k = 0; k < 3; ++k) a.hits[k] = hb ? hb + k * hits_stride : nullptr;
  // every cell's planes must keep the 16-byte alignment the vector stores need
  vec = vec && aligned16(hb) && (hits_stride * (int64_t)sizeof(T)) % 16 == 0;
  a.out = out8;
  a.status = status;
  a.n = n;
  a.first = 0;
  a.last = sys->n_surf - 1;
  a.n_wl = sys->n_wl;
  a.wl = 0;
  a.tiles_per_block = 1;
  ol::SpotBatch<T> b{};
  b.n_cells = n_cells;
  b.hits_stride = hits_stride;
  for (int c = 0; c < n_cells; ++c) {
    ol::RaygenIn<T> f = a.in;   // the launch-uniform field of this cell -> its tangents
    f.hx0 = (T)cells[c].hx;
    f.hy0 = (T)cells[c].hy;
    ol::uniform_field_tangents<T>(a.rg, f);
    b.c[c].tx = f.tx0;
    b.c[c].ty = f.ty0;
    b.c[c].vx = (T)cells[c].vx;
    b.c[c].vy = (T)cells[c].vy;
    b.c[c].cx = cells[c].cx;
    b.c[c].cy = cells[c].cy;
    b.c[c].wl = cells[c].wavelength_index;
    const ol_system* from = cells[c].optics_of ? cells[c].optics_of : sys;
    b.c[c].optics = table_of<T>(from).optics;
    b.c[c].n_wl = from->n_wl;
  }
  hipError_t e = ol::launch_spot_batch<T>(a, b, vec, newton_family(sys, 0, sys->n_surf - 1), stream);
  if (e != hipSuccess) return failf(OL_EHIP, "spot batch launch failed: %s", hipGetErrorString(e));
  return OL_OK;
}

template <typename T>
int do_wavefront_reference(const ol_system* sys, const DeviceTable<T>& tab,
                           const ol_raygen_params* p, const ol_raygen_inputs* in,
                           const ol_wavefront_params* w, double pupil_z, int32_t planar,
                           int32_t wl, void* reference_dev, void* chief8, uint32_t* status,
                           hipStream_t stream) {
  ol::ChiefArgs<T> a{};
  // launch-uniform field / vignetting only; the pupil point is (0, 0)
  a.in.hx = a.in.hy = a.in.px = a.in.py = a.in.vx = a.in.vy = nullptr;
  a.in.hx0 = (T)in->hx0; a.in.hy0 = (T)in->hy0; a.in.vx0 = (T)in->vx0; a.in.vy0 = (T)in->vy0;
  a.in.tx0 = a.in.ty0 = T(0);
  a.in.flags = in->flags & OL_RAYGEN_PRESCALE_PUPIL;
  a.surf = tab.surf;
  a.cold = tab.cold;
  a.optics = tab.optics;
  a.coeffs = tab.coeffs;
  a.rg = raygen_dev(p);
  ol::WavefrontDev wd{0, 0, 0, 0, w->n_image, 0, w->ux, w->uy, w->half_epd, w->wavelength_um,
                      0, 0, planar ? 1.0 : 0.0, w->last_thickness, w->last_absorb};
  a.wfc = ol::WavefrontConsts<T>(wd);   // planar flag from nz != 0; centre / R filled on device
  a.pupil_z = (T)pupil_z;
  a.out = static_cast<ol::WavefrontConsts<T>*>(reference_dev);
  a.chief = static_cast<T*>(chief8);
  a.status = status;
  a.first = 0;
  a.last = sys->n_surf - 1;
  a.n_wl = sys->n_wl;
  a.wl = wl;
  hipError_t e = ol::launch_chief_reference<T>(a, newton_family(sys, 0, sys->n_surf - 1), stream);
  if (e != hipSuccess)
    return failf(OL_EHIP, "chief-ray launch failed: %s", hipGetErrorString(e));
  return OL_OK;
}

template <typename T>
int do_trace_opd(const ol_system* sys, const DeviceTable<T>& tab, int64_t n,
                 const ol_raygen_params* p, const ol_raygen_inputs* in,
                 const ol_wavefront_params* w, int32_t wl, void* opd, void* inten,
                 void* const pupil[3], double* mom, uint32_t* status, hipStream_t stream,
                 const void* reference_dev = nullptr) {
  ol::OpdArgs<T> a{};
  a.wf_dev = static_cast<const ol::WavefrontConsts<T>*>(reference_dev);
  bool vec = true;
  if (int rc = convert_inputs<T>("ol_trace_opd", in, status, a.in, vec)) return rc;
  if (a.in.hx != nullptr || a.in.vx != nullptr)
    return failf(OL_EINVAL, "ol_trace_opd: one field point per launch (launch-uniform field and "
                            "vignetting, no hx / hy / vx / vy planes)");
  if (n == 0) return OL_OK;
  a.surf = tab.surf;
  a.cold = tab.cold;
  a.optics = tab.optics;
  a.coeffs = tab.coeffs;
  a.rg = raygen_dev(p);
  if (w)
    a.wf = ol::WavefrontDev{w->xc, w->yc, w->zc, w->R, w->n_image, w->opd_ref, w->ux, w->uy,
                            w->half_epd, w->wavelength_um, w->nx, w->ny, w->nz,
                            w->last_thickness, w->last_absorb};
  else
    a.wf = ol::WavefrontDev{0, 0, 0, 1, 1, 0, 0, 0, 1, 1, 0, 0, 0};  // (unused: reference_dev)
  a.opd = static_cast<T*>(opd);
  a.inten = static_cast<T*>(inten);
  for (int k = 0; k < 3; ++k) a.pupil[k] = pupil ? static_cast<T*>(pupil[k]) : nullptr;
  a.mom = mom;
  a.status = status;
  a.n = n;
  a.first = 0;
  a.last = sys->n_surf - 1;
  a.n_wl = sys->n_wl;
  a.wl = wl;
  vec = vec && aligned16(opd) && aligned16(inten);
  for (int k = 0; k < 3; ++k) vec = vec && aligned16(a.pupil[k]);
  hipError_t e =
      ol::launch_opd_trace<T>(a, vec, newton_family(sys, 0, sys->n_surf - 1), stream);
  if (e != hipSuccess) return failf(OL_EHIP, "opd launch failed: %s", hipGetErrorString(e));
  return OL_OK;
}

}  // namespace

// system_view.h: the fp64 table and the validation facts of a system for the entry points that
// live in translation units of their own (ray_aim.hip)
namespace ol {
SystemView system_view(const ol_system* sys) {
  return SystemView{sys->n_surf,        sys->n_wl,      sys->device,
                    sys->consistent,    sys->f64.surf,  sys->f64.cold,
                    sys->f64.optics,    sys->f64.coeffs, sys->facts.interaction.data(),
                    sys->facts.coating.data(), sys->facts.ref_newton.data(), sys->facts.geom.data(),
                    sys->f32.surf,      sys->f32.cold,  sys->f32.optics,
                    sys->f32.coeffs};
}
int system_newton_family(const ol_system* sys, int32_t first, int32_t last) {
  return newton_family(sys, first, last);
}
}  // namespace ol

extern "C" {

const char* ol_last_error(void) { return g_err.c_str(); }
int32_t ol_abi_version(void) { return OL_ABI_VERSION; }

int ol_set_tuning(int32_t knob, int32_t value) {
  switch (knob) {
    case OL_TUNE_RAYS_PER_THREAD:
      if (value < 0 || value > 3)
        return failf(OL_EINVAL, "ol_set_tuning: rays per thread must be 0 (auto), 1, 2 (vector) "
                                "or 3 (fp32 pair)");
      ol::tuning().rays_per_thread = value;
      return OL_OK;
    case OL_TUNE_COMPACT:
      ol::tuning().compact = value ? 1 : 0;
      return OL_OK;
    case OL_TUNE_RECORD_WG_CAP:
      if (value < 0 || value > 8)
        return failf(OL_EINVAL, "ol_set_tuning: record workgroup cap 0 (default policy), "
                                "1 (never) or 2 ... 8");
      ol::tuning().record_wg_cap = value;
      return OL_OK;
    case OL_TUNE_FIT_GRID:
      if (value < 0 || value > ol::kFitMaxBlocks)
        return failf(OL_EINVAL, "ol_set_tuning: fit grid 0 (default) ... %d", ol::kFitMaxBlocks);
      ol::tuning().fit_grid = value;
      return OL_OK;
    default:
      return failf(OL_EINVAL, "ol_set_tuning: unknown knob %d", knob);
  }
}

int ol_system_create(const ol_surface_desc* surf, int32_t n_surf, const double* coeffs,
                     int32_t n_coeffs, const ol_surface_optics* optics, int32_t n_wavelengths,
                     ol_system** out) {
  if (!out) return failf(OL_EINVAL, "ol_system_create: out is NULL");
  *out = nullptr;
  Staged st;
  if (int rc = stage_system("ol_system_create", surf, n_surf, coeffs, n_coeffs, optics,
                            n_wavelengths, st))
    return rc;
  ol_system* sys = new (std::nothrow) ol_system();
  if (!sys) return failf(OL_ENOMEM, "ol_system_create: out of host memory");
  sys->n_surf = n_surf;
  sys->n_wl = n_wavelengths;
  sys->facts = std::move(st.facts);
  if (!current_device(&sys->device)) {
    delete sys;
    return failf(OL_EHIP, "ol_system_create: no HIP device (hipGetDevice failed)");
  }
  int rc = upload<float>(st.surf, st.optics, st.coeffs, st.int_slots, sys->f32);
  if (rc == OL_OK) rc = upload<double>(st.surf, st.optics, st.coeffs, st.int_slots, sys->f64);
  if (rc != OL_OK) {
    release(sys->f32);
    release(sys->f64);
    delete sys;
    return rc;
  }
  *out = sys;
  return OL_OK;
}

int ol_system_update(ol_system* sys, const ol_surface_desc* surf, int32_t n_surf,
                     const double* coeffs, int32_t n_coeffs, const ol_surface_optics* optics,
                     int32_t n_wavelengths, void* stream) {
  if (!sys) return failf(OL_EINVAL, "ol_system_update: system is NULL");
  if (n_surf != sys->n_surf || n_wavelengths != sys->n_wl)
    return failf(OL_EUNSUPPORTED, "ol_system_update: %d surfaces x %d wavelengths do not fit the "
                                  "system's %d x %d tables", n_surf, n_wavelengths, sys->n_surf,
                 sys->n_wl);
  Staged st;
  if (int rc = stage_system("ol_system_update", surf, n_surf, coeffs, n_coeffs, optics,
                            n_wavelengths, st))
    return rc;
  if (int rc = rule_consistent("ol_system_update", sys->consistent)) return rc;
  const size_t need = st.coeffs.size() ? st.coeffs.size() : 1;
  if (need > sys->f32.coef_capacity || need > sys->f64.coef_capacity)
    return failf(OL_EUNSUPPORTED, "ol_system_update: coefficient block of %zu values exceeds the "
                                  "allocated %zu", need, sys->f32.coef_capacity);
  if (int rc = rule_current_device("ol_system_update", system_view(sys))) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // the fp64 table first: if its copy fails nothing has changed yet and the system stays
  // usable; only a failure of the SECOND copy leaves the two precisions apart
  int rc = upload<double>(st.surf, st.optics, st.coeffs, st.int_slots, sys->f64, true, s);
  if (rc != OL_OK) return rc;
  sys->consistent = false;
  rc = upload<float>(st.surf, st.optics, st.coeffs, st.int_slots, sys->f32, true, s);
  if (rc != OL_OK) return rc;
  sys->facts = std::move(st.facts);
  sys->consistent = true;
  return OL_OK;
}

void ol_system_destroy(ol_system* sys) {
  if (!sys) return;
  release(sys->f32);
  release(sys->f64);
  delete sys;
}

int32_t ol_system_num_surfaces(const ol_system* sys) { return sys ? sys->n_surf : 0; }

int ol_trace(const ol_system* sys, ol_dtype dt, int64_t n_rays, void* const rays[8],
             int32_t wavelength_index, void* record, int64_t record_stride, void* prt,
             int32_t first_surface, int32_t last_surface, uint32_t flags, uint32_t* status,
             void* stream) {
  return ol_trace_ex(sys, dt, n_rays, rays, wavelength_index, record, record_stride, prt,
                     first_surface, last_surface, flags, status, nullptr, stream);
}

int ol_trace_ex(const ol_system* sys, ol_dtype dt, int64_t n_rays, void* const rays[8],
                int32_t wavelength_index, void* record, int64_t record_stride, void* prt,
                int32_t first_surface, int32_t last_surface, uint32_t flags, uint32_t* status,
                const ol_trace_extras* extras, void* stream) {
  SystemView v;
  if (int rc = rule_system("ol_trace", sys, v)) return rc;
  if (int rc = rule_dtype("ol_trace", dt)) return rc;
  if (int rc = rule_count("ol_trace", n_rays, "negative ray count")) return rc;
  if (int rc = rule_range("ol_trace", v, first_surface, last_surface)) return rc;
  if (int rc = rule_wavelength("ol_trace", v.n_wl, wavelength_index)) return rc;
  if (int rc = rule_no_single_kinds("ol_trace", v, first_surface, last_surface)) return rc;
  if (n_rays == 0) return OL_OK;
  if (int rc = rule_current_device("ol_trace", v)) return rc;
  if (int rc = rule_planes("ol_trace", "rays", rays, 8)) return rc;
  if (record)
    if (int rc = rule_stride("ol_trace", record_stride, n_rays)) return rc;
  if (!record && !(flags & OL_TRACE_WRITE_RAYS) && !prt && !(extras && extras->spot_slots))
    return failf(OL_EINVAL, "ol_trace: nothing to write (no record, no OL_TRACE_WRITE_RAYS)");
  if (extras && extras->record_first_surface > last_surface)
    return failf(OL_EINVAL, "ol_trace_ex: record_first_surface %d beyond last_surface %d",
                 extras->record_first_surface, last_surface);
  if (prt && extras && extras->spot_slots)
    return failf(OL_EINVAL, "ol_trace_ex: the spot epilogue is for unpolarised traces (the "
                            "polarised intensity needs ol_polarized_intensity first)");
  if (!prt)
    if (int rc = rule_polarisation_required(v, first_surface, last_surface)) return rc;
  if (prt && !(flags & OL_TRACE_PRT_COMPLEX))
    if (int rc = rule_retarder_needs_complex("ol_trace", v, first_surface, last_surface)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return by_dtype(dt, sys, [&](auto zero, const auto& table) {
    return do_trace<decltype(zero)>(sys, table, n_rays, rays, wavelength_index, record,
                                    record_stride, prt, first_surface, last_surface, flags, status,
                                    extras, st);
  });
}

int ol_newton_count(const ol_system* sys, ol_dtype dt, int64_t n_rays, void* const rays[8],
                    int32_t wavelength_index, int32_t first_surface, int32_t surface,
                    int32_t* iterations, int32_t verify, void* stream) {
  SystemView v;
  if (int rc = rule_system("ol_newton_count", sys, v)) return rc;
  if (int rc = rule_dtype("ol_newton_count", dt)) return rc;
  if (int rc = rule_count("ol_newton_count", n_rays, "negative ray count")) return rc;
  if (int rc = rule_range("ol_newton_count", v, first_surface, surface)) return rc;
  if (int rc = rule_wavelength("ol_newton_count", v.n_wl, wavelength_index)) return rc;
  if (!iterations) return failf(OL_EINVAL, "ol_newton_count: iterations is NULL");
  if (int rc = rule_no_single_kinds("ol_newton_count", v, first_surface, surface)) return rc;
  if (!v.ref_newton[surface])
    return failf(OL_EINVAL, "ol_newton_count: surface %d is not a traced Newton-Raphson surface "
                            "with OL_SURF_REFERENCE_NEWTON", surface);
  if (n_rays == 0) return OL_OK;
  if (int rc = rule_current_device("ol_newton_count", v)) return rc;
  if (int rc = rule_planes("ol_newton_count", "rays", rays, 8)) return rc;
  // the geometry of a ray does not depend on its polarisation: the unpolarised kernel over
  // [first_surface, surface], nothing recorded, nothing written back
  ol_trace_extras ex{};
  ex.newton_iterations = iterations;
  ex.newton_count_surface = verify ? -1 : surface;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return by_dtype(dt, sys, [&](auto zero, const auto& table) {
    return do_trace<decltype(zero)>(sys, table, n_rays, rays, wavelength_index, nullptr, 0,
                                    nullptr, first_surface, surface, 0u, nullptr, &ex, st);
  });
}

int ol_trace_generate(const ol_system* sys, ol_dtype dt, int64_t n_rays,
                      const ol_raygen_params* p, const ol_raygen_inputs* in,
                      int32_t wavelength_index, void* record, int64_t record_stride,
                      void* const rays_out[8], void* prt, uint32_t flags, uint32_t* status,
                      const ol_trace_extras* extras, void* stream) {
  SystemView v;
  if (int rc = rule_system("ol_trace_generate", sys, v)) return rc;
  if (int rc = rule_no_reference_newton("ol_trace_generate", v)) return rc;
  if (int rc = rule_dtype("ol_trace_generate", dt)) return rc;
  if (!p || !in) return failf(OL_EINVAL, "ol_trace_generate: NULL argument");
  if (int rc = rule_count("ol_trace_generate", n_rays, "negative ray count")) return rc;
  if (int rc = rule_wavelength("ol_trace_generate", v.n_wl, wavelength_index)) return rc;
  if ((in->vx || in->vy) && !(in->hx && in->hy))
    return failf(OL_EUNSUPPORTED, "ol_trace_generate: per-ray vignetting planes come with "
                                  "per-ray field planes (else ol_generate_rays + ol_trace)");
  // (ABI 10: polarised launches take per-ray field planes and apodized pupils too)
  if (extras && extras->spot_slots) {
    if (prt)
      return failf(OL_EINVAL, "ol_trace_generate: the spot epilogue is for unpolarised traces "
                              "(the polarised intensity needs update_intensity first)");
    if (in->hx || in->hy || p->apod_kind != OL_APOD_NONE)
      return failf(OL_EUNSUPPORTED, "ol_trace_generate: the spot epilogue is one field point "
                                    "without apodization (else ol_trace_spot)");
    if (extras->record_first_surface > 0)
      return failf(OL_EINVAL, "ol_trace_generate: spot epilogue and record_first_surface "
                              "cannot be combined");
  }
  if (!record) return failf(OL_EINVAL, "ol_trace_generate: record is NULL");
  if (int rc = rule_stride("ol_trace_generate", record_stride, n_rays)) return rc;
  if (extras && extras->record_first_surface >= sys->n_surf)
    return failf(OL_EINVAL, "ol_trace_generate: record_first_surface %d outside [0, %d)",
                 extras->record_first_surface, sys->n_surf);
  if (rays_out)
    if (int rc = rule_planes("ol_trace_generate", "rays_out", rays_out, 8)) return rc;
  if (!prt)
    if (int rc = rule_polarisation_required(v, 0, v.n_surf - 1)) return rc;
  if (prt && !(flags & OL_TRACE_PRT_COMPLEX))
    if (int rc = rule_retarder_needs_complex("ol_trace_generate", v, 0, v.n_surf - 1)) return rc;
  if (n_rays > 0)
    if (int rc = rule_current_device("ol_trace_generate", v)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return by_dtype(dt, sys, [&](auto zero, const auto& table) {
    return do_trace_generate<decltype(zero)>(sys, table, n_rays, p, in, wavelength_index, record,
                                             record_stride, rays_out, prt, flags, status, extras,
                                             st);
  });
}

int ol_generate_rays(const ol_raygen_params* p, ol_dtype dt, int64_t n,
                     const ol_raygen_inputs* in, void* const out[8], uint32_t* status,
                     void* stream) {
  if (!p || !in || !out) return failf(OL_EINVAL, "ol_generate_rays: NULL argument");
  if (int rc = rule_count("ol_generate_rays", n, "negative count")) return rc;
  if (n > 0)
    if (int rc = rule_planes("ol_generate_rays", "out", out, 7)) return rc;
  if (int rc = rule_dtype("ol_generate_rays", dt)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return by_dtype(dt, [&](auto zero) {
    return do_generate_rays<decltype(zero)>(p, n, in, out, status, st);
  });
}

int ol_trace_spot(const ol_system* sys, ol_dtype dt, int64_t n_rays, const ol_raygen_params* p,
                  const ol_raygen_inputs* in, double cx, double cy, int32_t wavelength_index,
                  void* const hits[3], double* out7, uint32_t* status, void* stream) {
  SystemView v;
  if (int rc = rule_system("ol_trace_spot", sys, v)) return rc;
  if (int rc = rule_no_reference_newton("ol_trace_spot", v)) return rc;
  if (int rc = rule_dtype("ol_trace_spot", dt)) return rc;
  if (!p || !in || !out7) return failf(OL_EINVAL, "ol_trace_spot: NULL argument");
  if (hits && (!hits[0] || !hits[1] || !hits[2]))
    return failf(OL_EINVAL, "ol_trace_spot: hits needs three planes");
  if (int rc = rule_count("ol_trace_spot", n_rays, "negative ray count")) return rc;
  if (int rc = rule_wavelength("ol_trace_spot", v.n_wl, wavelength_index)) return rc;
  if (!(in->flags & OL_SPOT_POLARIZED_OK))
    if (int rc = rule_polarisation_required(v, 0, v.n_surf - 1)) return rc;
  if (n_rays > 0)
    if (int rc = rule_current_device("ol_trace_spot", v)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return by_dtype(dt, sys, [&](auto zero, const auto& table) {
    return do_trace_spot<decltype(zero)>(sys, table, n_rays, p, in, cx, cy, wavelength_index, hits,
                                         out7, status, st);
  });
}

int ol_trace_spot_batch(const ol_system* sys, ol_dtype dt, int64_t n_rays, const ol_raygen_params* p,
                        const ol_raygen_inputs* in, int32_t n_cells, const ol_spot_cell* cells,
                        void* hits, int64_t hits_stride, double* out8, uint32_t* status,
                        void* stream) {
  SystemView v;
  if (int rc = rule_system("ol_trace_spot_batch", sys, v)) return rc;
  if (int rc = rule_no_reference_newton("ol_trace_spot_batch", v)) return rc;
  if (int rc = rule_dtype("ol_trace_spot_batch", dt)) return rc;
  if (!p || !in || !out8 || (n_cells > 0 && !cells))
    return failf(OL_EINVAL, "ol_trace_spot_batch: NULL argument");
  if (int rc = rule_count("ol_trace_spot_batch", n_rays, "negative ray count")) return rc;
  if (n_cells < 0 || n_cells > OL_SPOT_BATCH_MAX_CELLS)
    return failf(OL_EINVAL, "ol_trace_spot_batch: %d cells outside [0, %d]", n_cells,
                 OL_SPOT_BATCH_MAX_CELLS);
  if (in->hx || in->hy || in->vx || in->vy)
    return failf(OL_EINVAL, "ol_trace_spot_batch: per-ray field / vignetting planes with cells "
                            "(each cell has ONE field point)");
  if (hits && hits_stride < n_rays)
    return failf(OL_EINVAL, "ol_trace_spot_batch: hits_stride %lld < %lld rays",
                 (long long)hits_stride, (long long)n_rays);
  for (int32_t c = 0; c < n_cells; ++c) {
    const ol_system* from = cells[c].optics_of ? cells[c].optics_of : sys;
    if (from != sys) {
      if (int rc = rule_consistent("ol_trace_spot_batch (optics_of)", from->consistent)) return rc;
      if (from->n_surf != sys->n_surf || from->device != sys->device)
        return failf(OL_EINVAL, "ol_trace_spot_batch: cell %d: optics_of has %d surfaces on device "
                                "%d, the system %d on device %d", c, from->n_surf, from->device,
                     sys->n_surf, sys->device);
    }
    char who[48];
    snprintf(who, sizeof(who), "ol_trace_spot_batch: cell %d", c);
    if (int rc = rule_wavelength(who, from->n_wl, cells[c].wavelength_index)) return rc;
    if (in->flags & OL_RAYGEN_CHECK_FIELD) {
      auto bad = [](double v) { return !(v >= -1.0 && v <= 1.0); };
      if (bad(cells[c].hx) || bad(cells[c].hy))  // real_ray_tracer.py:156-173, same text
        return failf(OL_EINVAL, "Normalized field coordinates must be within (-1, 1)");
    }
  }
  if (!(in->flags & OL_SPOT_POLARIZED_OK))
    if (int rc = rule_polarisation_required(v, 0, v.n_surf - 1)) return rc;
  if (n_rays > 0 && n_cells > 0)
    if (int rc = rule_current_device("ol_trace_spot_batch", v)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return by_dtype(dt, sys, [&](auto zero, const auto& table) {
    return do_trace_spot_batch<decltype(zero)>(sys, table, n_rays, p, in, n_cells, cells, hits,
                                               hits_stride, out8, status, st);
  });
}

int ol_irradiance(ol_dtype dt, int64_t n_rays, const void* x, const void* y, const void* power,
                  const double* x_edges, int32_t nx, const double* y_edges, int32_t ny,
                  double* hist, void* stream) {
  if (!x || !y || !power || !x_edges || !y_edges || !hist)
    return failf(OL_EINVAL, "ol_irradiance: NULL argument");
  if (int rc = rule_count("ol_irradiance", n_rays, "negative count")) return rc;
  if (nx < 1 || ny < 1 || (int64_t)nx * ny > (int64_t)1 << 28)
    return failf(OL_EINVAL, "ol_irradiance: %d x %d bins", nx, ny);
  if (n_rays == 0) return OL_OK;
  if (int rc = rule_dtype("ol_irradiance", dt)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const hipError_t e = by_dtype(dt, [&](auto zero) {
    using T = decltype(zero);
    return ol::launch_irradiance<T>(n_rays, (const T*)x, (const T*)y, (const T*)power, x_edges, nx,
                                    y_edges, ny, hist, st);
  });
  if (e != hipSuccess) return failf(OL_EHIP, "launch failed: %s", hipGetErrorString(e));
  return OL_OK;
}

int ol_radial_energy(ol_dtype dt, int64_t n_rays, const void* x, const void* y,
                     const void* intensity, double cx, double cy, const double* r_step,
                     int32_t n_steps, double* bins, void* stream) {
  if (!x || !y || !intensity || !r_step || !bins)
    return failf(OL_EINVAL, "ol_radial_energy: NULL argument");
  if (int rc = rule_count("ol_radial_energy", n_rays, "negative count")) return rc;
  if (n_steps < 1 || n_steps > 1024)
    return failf(OL_EINVAL, "ol_radial_energy: n_steps %d outside [1, 1024]", n_steps);
  if (n_rays == 0) return OL_OK;
  if (int rc = rule_dtype("ol_radial_energy", dt)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const hipError_t e = by_dtype(dt, [&](auto zero) {
    using T = decltype(zero);
    return ol::launch_radial_energy<T>(n_rays, (const T*)x, (const T*)y, (const T*)intensity, cx,
                                       cy, r_step, n_steps, bins, st);
  });
  if (e != hipSuccess) return failf(OL_EHIP, "launch failed: %s", hipGetErrorString(e));
  return OL_OK;
}

int ol_polarized_intensity(ol_dtype dt, int64_t n_rays, const void* prt, int32_t prt_complex,
                           const void* const k0[3], const void* i0,
                           const ol_polarization_state* state, void* intensity,
                           uint32_t* status, void* stream) {
  if (!prt || !k0 || !k0[0] || !k0[1] || !k0[2] || !i0 || !state || !intensity)
    return failf(OL_EINVAL, "ol_polarized_intensity: NULL argument");
  if (int rc = rule_count("ol_polarized_intensity", n_rays, "negative count")) return rc;
  if (n_rays == 0) return OL_OK;
  ol::PolStateDev s{state->is_polarized, state->Ex, state->Ey, state->phase_x, state->phase_y};
  if (int rc = rule_dtype("ol_polarized_intensity", dt)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const hipError_t e = by_dtype(dt, [&](auto zero) {
    using T = decltype(zero);
    const T* k[3] = {(const T*)k0[0], (const T*)k0[1], (const T*)k0[2]};
    return ol::launch_pol_intensity<T>(n_rays, (const T*)prt, prt_complex != 0, k, (const T*)i0, s,
                                       (T*)intensity, status, st);
  });
  if (e != hipSuccess) return failf(OL_EHIP, "launch failed: %s", hipGetErrorString(e));
  return OL_OK;
}

int ol_wavefront_opd(const ol_wavefront_params* p, ol_dtype dt, int64_t n_rays,
                     const void* const rays[7], const void* px, const void* py,
                     void* opd_waves, void* const pupil[3], void* stream) {
  if (!p || !rays || !px || !py || !opd_waves)
    return failf(OL_EINVAL, "ol_wavefront_opd: NULL argument");
  if (int rc = rule_count("ol_wavefront_opd", n_rays, "negative count")) return rc;
  if (n_rays == 0) return OL_OK;
  if (int rc = rule_planes("ol_wavefront_opd", "rays", rays, 7)) return rc;
  if (pupil && (!pupil[0] || !pupil[1] || !pupil[2]))
    return failf(OL_EINVAL, "ol_wavefront_opd: pupil planes must all be given or pupil = NULL");
  ol::WavefrontDev d{p->xc, p->yc, p->zc, p->R, p->n_image, p->opd_ref,
                     p->ux, p->uy, p->half_epd, p->wavelength_um, p->nx, p->ny, p->nz};
  if (int rc = rule_dtype("ol_wavefront_opd", dt)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const hipError_t e = by_dtype(dt, [&](auto zero) {
    using T = decltype(zero);
    const T* r[7];
    for (int k = 0; k < 7; ++k) r[k] = static_cast<const T*>(rays[k]);
    T* pu[3] = {pupil ? (T*)pupil[0] : nullptr, pupil ? (T*)pupil[1] : nullptr,
                pupil ? (T*)pupil[2] : nullptr};
    return ol::launch_wavefront<T>(d, n_rays, r, (const T*)px, (const T*)py, (T*)opd_waves,
                                   pupil ? pu : nullptr, st);
  });
  if (e != hipSuccess) return failf(OL_EHIP, "launch failed: %s", hipGetErrorString(e));
  return OL_OK;
}

int ol_trace_opd(const ol_system* sys, ol_dtype dt, int64_t n_rays, const ol_raygen_params* p,
                 const ol_raygen_inputs* in, const ol_wavefront_params* w,
                 int32_t wavelength_index, void* opd_waves, void* intensity,
                 void* const pupil[3], double* moments12, uint32_t* status, void* stream) {
  SystemView v;
  if (int rc = rule_system("ol_trace_opd", sys, v)) return rc;
  if (int rc = rule_no_reference_newton("ol_trace_opd", v)) return rc;
  if (dt != OL_F64)
    return failf(dt == OL_F32 ? OL_EUNSUPPORTED : OL_EINVAL,
                 "ol_trace_opd: wavefront work is fp64 only (dtype %d)", (int)dt);
  if (!p || !in || !w || !opd_waves || !intensity || !moments12)
    return failf(OL_EINVAL, "ol_trace_opd: NULL argument");
  if (pupil && (!pupil[0] || !pupil[1] || !pupil[2]))
    return failf(OL_EINVAL, "ol_trace_opd: pupil planes must all be given or pupil = NULL");
  if (int rc = rule_count("ol_trace_opd", n_rays, "negative ray count")) return rc;
  if (int rc = rule_wavelength("ol_trace_opd", v.n_wl, wavelength_index)) return rc;
  if (int rc = rule_polarisation_required(v, 0, v.n_surf - 1)) return rc;
  if (n_rays > 0)
    if (int rc = rule_current_device("ol_trace_opd", v)) return rc;
  return do_trace_opd<double>(sys, sys->f64, n_rays, p, in, w, wavelength_index, opd_waves,
                              intensity, pupil, moments12, status,
                              static_cast<hipStream_t>(stream));
}

// what ol_wavefront_reference and ol_trace_opd_dev check first, in this order
static int opd_common_checks(const char* who, const ol_system* sys, ol_dtype dt,
                             int32_t wavelength_index) {
  SystemView v;
  if (int rc = rule_system(who, sys, v)) return rc;
  if (int rc = rule_fp64_only(who, dt)) return rc;
  if (int rc = rule_wavelength(who, v.n_wl, wavelength_index)) return rc;
  if (int rc = rule_no_reference_newton(who, v)) return rc;
  if (int rc = rule_polarisation_required(v, 0, v.n_surf - 1)) return rc;
  return rule_current_device(who, v);
}

int ol_wavefront_reference(const ol_system* sys, ol_dtype dt, const ol_raygen_params* p,
                           const ol_raygen_inputs* in, const ol_wavefront_params* w,
                           double pupil_z, int32_t planar, int32_t wavelength_index,
                           void* reference_dev, void* chief8, uint32_t* status, void* stream) {
  if (int rc = opd_common_checks("ol_wavefront_reference", sys, dt, wavelength_index)) return rc;
  if (!p || !in || !w || !reference_dev)
    return failf(OL_EINVAL, "ol_wavefront_reference: NULL argument");
  if (in->hx || in->hy || in->vx || in->vy)
    return failf(OL_EINVAL, "ol_wavefront_reference: one field point (launch-uniform field and "
                            "vignetting)");
  return do_wavefront_reference<double>(sys, sys->f64, p, in, w, pupil_z, planar,
                                        wavelength_index, reference_dev, chief8, status,
                                        static_cast<hipStream_t>(stream));
}

int ol_trace_opd_dev(const ol_system* sys, ol_dtype dt, int64_t n_rays,
                     const ol_raygen_params* p, const ol_raygen_inputs* in,
                     const void* reference_dev, int32_t wavelength_index, void* opd_waves,
                     void* intensity, void* const pupil[3], double* moments12, uint32_t* status,
                     void* stream) {
  if (int rc = opd_common_checks("ol_trace_opd_dev", sys, dt, wavelength_index)) return rc;
  if (!p || !in || !reference_dev || !opd_waves || !intensity || !moments12)
    return failf(OL_EINVAL, "ol_trace_opd_dev: NULL argument");
  if (pupil && (!pupil[0] || !pupil[1] || !pupil[2]))
    return failf(OL_EINVAL, "ol_trace_opd_dev: pupil needs three planes");
  if (int rc = rule_count("ol_trace_opd_dev", n_rays, "negative ray count")) return rc;
  return do_trace_opd<double>(sys, sys->f64, n_rays, p, in, nullptr, wavelength_index, opd_waves,
                              intensity, pupil, moments12, status,
                              static_cast<hipStream_t>(stream), reference_dev);
}

int ol_wavefront_fit(int32_t kind, const ol_wavefront_params* w, double trim_std,
                     uint32_t flags, int32_t planar, int64_t n_rays,
                     const double* const rays[8], const double* px, const double* py,
                     double* workspace, void* reference_dev, uint32_t* fit_status,
                     void* stream) {
  static_assert(OL_WAVEFRONT_FIT_WORKSPACE_DOUBLES == ol::kFitWorkspaceDoubles, "header");
  static_assert(sizeof(ol::WavefrontConsts<double>) <= OL_WAVEFRONT_REFERENCE_DOUBLES * 8,
                "header: the device reference structure");
  static_assert(OL_FIT_NO_VALID == ol::kFitNoValid && OL_FIT_TOO_FEW == ol::kFitTooFew &&
                OL_FIT_NO_ALIVE == ol::kFitNoAlive && OL_FIT_SINGULAR == ol::kFitSingular &&
                OL_FIT_CENTROID == ol::kFitCentroid && OL_FIT_BEST_FIT == ol::kFitBestFit,
                "header");
  if (!w || !rays || !px || !py || !workspace || !reference_dev || !fit_status)
    return failf(OL_EINVAL, "ol_wavefront_fit: NULL argument");
  if (kind != OL_FIT_CENTROID && kind != OL_FIT_BEST_FIT)
    return failf(OL_EINVAL, "ol_wavefront_fit: unknown kind %d", (int)kind);
  if (int rc = rule_count("ol_wavefront_fit", n_rays, "negative count")) return rc;
  if (flags & ~(uint32_t)(OL_FIT_STD_DDOF1 | OL_FIT_PISTON_SKIPS_NAN))
    return failf(OL_EINVAL, "ol_wavefront_fit: unknown flags 0x%x", (unsigned)flags);
  if (!(w->n_image > 0.0) || !(w->wavelength_um > 0.0))
    return failf(OL_EINVAL, "ol_wavefront_fit: n_image %g, wavelength %g", w->n_image,
                 w->wavelength_um);
  if (int rc = rule_planes("ol_wavefront_fit", "rays", rays, 8)) return rc;
  ol::FitArgs a{};
  a.p.ni = w->n_image;
  a.p.inv_w = 1.0 / (w->wavelength_um * 1e-3);
  a.p.ux = w->ux;
  a.p.uy = w->uy;
  a.p.half_epd = w->half_epd;
  a.p.trim_std = trim_std > 0.0 ? trim_std : 0.0;  // (NaN: no trimming either)
  a.p.kind = kind;
  a.p.planar = planar ? 1 : 0;
  a.p.ddof = (flags & OL_FIT_STD_DDOF1) ? 1 : 0;
  a.p.skip_nan = (flags & OL_FIT_PISTON_SKIPS_NAN) ? 1 : 0;
  for (int k = 0; k < 8; ++k) a.ray[k] = rays[k];
  a.px = px;
  a.py = py;
  a.n = n_rays;
  a.workspace = workspace;
  a.out = static_cast<ol::WavefrontConsts<double>*>(reference_dev);
  a.status = fit_status;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = ol::launch_wavefront_fit(a, st);  // (its first pass writes fit_status)
  if (e != hipSuccess) return failf(OL_EHIP, "ol_wavefront_fit: %s", hipGetErrorString(e));
  return OL_OK;
}

int ol_wavefront_opd_fitted(int64_t n_rays, const double* const rays[7], const double* px,
                            const double* py, const void* reference_dev, double* opd_waves,
                            double* const pupil[3], void* stream) {
  if (!rays || !px || !py || !reference_dev || !opd_waves)
    return failf(OL_EINVAL, "ol_wavefront_opd_fitted: NULL argument");
  if (int rc = rule_count("ol_wavefront_opd_fitted", n_rays, "negative count")) return rc;
  if (int rc = rule_planes("ol_wavefront_opd_fitted", "rays", rays, 7)) return rc;
  if (pupil && (!pupil[0] || !pupil[1] || !pupil[2]))
    return failf(OL_EINVAL, "ol_wavefront_opd_fitted: pupil needs three planes");
  if (n_rays == 0) return OL_OK;
  hipError_t e = ol::launch_wavefront_fitted(
      static_cast<const ol::WavefrontConsts<double>*>(reference_dev), n_rays, rays, px, py,
      opd_waves, pupil, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return failf(OL_EHIP, "ol_wavefront_opd_fitted: %s", hipGetErrorString(e));
  return OL_OK;
}

int ol_pupil_fill(ol_dtype dt, int64_t n_rays, const void* opd_waves, const void* intensity,
                  const void* pupil_x, const void* pupil_y, const double plane[3],
                  const int32_t* cell, int32_t n_side, int32_t grid_size, double* grid,
                  void* stream) {
  if (!opd_waves || !intensity || !cell || !grid)
    return failf(OL_EINVAL, "ol_pupil_fill: NULL argument");
  if ((pupil_x == nullptr) != (pupil_y == nullptr) || (pupil_x && !plane))
    return failf(OL_EINVAL, "ol_pupil_fill: pupil_x, pupil_y and plane go together");
  if (n_rays < 0 || n_side < 1 || grid_size < n_side || grid_size > (1 << 15))
    return failf(OL_EINVAL, "ol_pupil_fill: n_rays %lld, %d samples per side, grid %d",
                 (long long)n_rays, n_side, grid_size);
  if (n_rays > (int64_t)n_side * n_side)
    return failf(OL_EINVAL, "ol_pupil_fill: more samples than cells");
  if (n_rays == 0) return OL_OK;
  const double zero[3] = {0.0, 0.0, 0.0};
  const double* co = plane ? plane : zero;
  const int32_t pad = (grid_size - n_side) / 2;  // psf/fft.py:139-160
  if (int rc = rule_dtype("ol_pupil_fill", dt)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const hipError_t e = by_dtype(dt, [&](auto zero) {
    using T = decltype(zero);
    return ol::launch_pupil_fill<T>(n_rays, (const T*)opd_waves, (const T*)intensity,
                                    (const T*)pupil_x, (const T*)pupil_y, co, cell, n_side,
                                    grid_size, pad, grid, st);
  });
  if (e != hipSuccess) return failf(OL_EHIP, "launch failed: %s", hipGetErrorString(e));
  return OL_OK;
}

int ol_pupil_points(int32_t kind, int32_t param, ol_dtype dt, int64_t n_points,
                    const int32_t* row_first, const int64_t* row_offset, void* x, void* y,
                    void* stream) {
  if (kind != OL_PUPIL_HEXAPOLAR && kind != OL_PUPIL_UNIFORM)
    return failf(OL_EINVAL, "ol_pupil_points: unknown sampler %d", kind);
  if (n_points < 0 || (n_points > 0 && (!x || !y)))
    return failf(OL_EINVAL, "ol_pupil_points: bad output planes");
  if (kind == OL_PUPIL_HEXAPOLAR) {
    if (param < 0 || n_points != 1 + 3 * (int64_t)param * ((int64_t)param + 1))
      return failf(OL_EINVAL, "ol_pupil_points: %d rings are %lld points, not %lld", param,
                   (long long)(1 + 3 * (int64_t)param * ((int64_t)param + 1)),
                   (long long)n_points);
  } else {
    if (param < 2) return failf(OL_EINVAL, "ol_pupil_points: uniform grid side %d < 2", param);
    if (n_points > 0 && (!row_first || !row_offset))
      return failf(OL_EINVAL, "ol_pupil_points: the uniform sampler needs its row tables");
  }
  if (int rc = rule_dtype("ol_pupil_points", dt)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const hipError_t e = by_dtype(dt, [&](auto zero) {
    using T = decltype(zero);
    return ol::launch_pupil_points<T>(kind, param, n_points, row_first, row_offset,
                                      static_cast<T*>(x), static_cast<T*>(y), st);
  });
  if (e != hipSuccess) return failf(OL_EHIP, "pupil launch failed: %s", hipGetErrorString(e));
  return OL_OK;
}

int ol_math_probe(int32_t op, ol_dtype dt, int64_t n, const void* a, const void* b, void* out,
                  void* stream) {
  if (op < 0 || op > 3) return failf(OL_EINVAL, "ol_math_probe: op must be 0..3");
  if (n < 0 || (n > 0 && (!a || !out || (op == 1 && !b))))
    return failf(OL_EINVAL, "ol_math_probe: NULL argument");
  if (int rc = rule_dtype("ol_math_probe", dt)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const hipError_t e = by_dtype(dt, [&](auto zero) {
    using T = decltype(zero);
    return ol::launch_math_probe<T>(op, n, static_cast<const T*>(a), static_cast<const T*>(b),
                                    static_cast<T*>(out), st);
  });
  if (e != hipSuccess) return failf(OL_EHIP, "probe launch failed: %s", hipGetErrorString(e));
  return OL_OK;
}

int ol_stream_fill(void* dst, int64_t bytes, int32_t store_bytes, int32_t planes,
                   uint32_t pattern, void* stream) {
  if (bytes < 0 || (bytes > 0 && !dst)) return failf(OL_EINVAL, "ol_stream_fill: bad buffer");
  if (planes < 1) return failf(OL_EINVAL, "ol_stream_fill: planes must be >= 1");
  if (store_bytes != 4 && store_bytes != 8 && store_bytes != 16)
    return failf(OL_EINVAL, "ol_stream_fill: store_bytes must be 4, 8 or 16");
  if (bytes % ((int64_t)store_bytes * planes) != 0 ||
      (reinterpret_cast<uintptr_t>(dst) % store_bytes) != 0)
    return failf(OL_EINVAL, "ol_stream_fill: buffer not a multiple of planes x store_bytes, or "
                            "not aligned to store_bytes");
  hipError_t e = ol::launch_stream_fill(dst, bytes, store_bytes, planes, pattern,
                                        static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return failf(OL_EHIP, "fill launch failed: %s", hipGetErrorString(e));
  return OL_OK;
}

int ol_arena_alloc(int64_t bytes, void** out) {
  if (!out) return failf(OL_EINVAL, "ol_arena_alloc: out is NULL");
  *out = nullptr;
  if (bytes <= 0) return failf(OL_EINVAL, "ol_arena_alloc: %lld bytes", (long long)bytes);
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, (size_t)bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();  // (an out-of-memory answer is not a sticky error)
    return failf(OL_EHIP, "ol_arena_alloc: %lld bytes: %s", (long long)bytes,
                 hipGetErrorString(e));
  }
  *out = p;
  return OL_OK;
}

int ol_arena_free(void* arena) {
  if (!arena) return OL_OK;
  hipError_t e = hipFree(arena);
  if (e != hipSuccess) return failf(OL_EHIP, "ol_arena_free: %s", hipGetErrorString(e));
  return OL_OK;
}

int ol_spot_moments(ol_dtype dt, int64_t n_rays, const void* x, const void* y,
                    const void* intensity, double* out6, void* stream) {
  if (!x || !y || !intensity || !out6) return failf(OL_EINVAL, "ol_spot_moments: NULL argument");
  if (int rc = rule_count("ol_spot_moments", n_rays, "negative count")) return rc;
  if (n_rays == 0) return OL_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const hipError_t e = by_dtype(dt, [&](auto zero) {
    using T = decltype(zero);
    return ol::launch_spot_moments<T>(n_rays, (const T*)x, (const T*)y, (const T*)intensity, out6,
                                      st);
  });
  if (e != hipSuccess) return failf(OL_EHIP, "launch failed: %s", hipGetErrorString(e));
  return OL_OK;
}

int ol_spot_max_r2(ol_dtype dt, int64_t n_rays, const void* x, const void* y,
                   const void* intensity, double cx, double cy, double* out1, void* stream) {
  if (!x || !y || !intensity || !out1) return failf(OL_EINVAL, "ol_spot_max_r2: NULL argument");
  if (int rc = rule_count("ol_spot_max_r2", n_rays, "negative count")) return rc;
  if (n_rays == 0) return OL_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const hipError_t e = by_dtype(dt, [&](auto zero) {
    using T = decltype(zero);
    return ol::launch_spot_max_r2<T>(n_rays, (const T*)x, (const T*)y, (const T*)intensity, cx, cy,
                                     out1, st);
  });
  if (e != hipSuccess) return failf(OL_EHIP, "launch failed: %s", hipGetErrorString(e));
  return OL_OK;
}

}  // extern "C"
