// ensemble.hip -- K variants of one optic traced and reduced to spot moments in ONE launch
// (ol_ensemble_*, ol_trace_spot_ensemble).
//
// Reference: tolerancing/monte_carlo.py -- per iteration every perturbation is applied and the
// operands (optimization/operand/ray.py: rms_spot_size) trace a few hundred rays through the
// perturbed lens.  On the device one such trace is a launch-bound kernel of ~0.15 ms behind a table
// upload, and the kernel that would do the work sits idle.  Here the variants live on the device
// together (stacked tables, ensemble_device.h) and the launch grid is
//   blockIdx.x   block of ray tiles       blockIdx.y, blockIdx.z   the cell (variant, field,
//                                                                   wavelength): any number of them
// so everything a cell changes -- the variant's table rows and ray-generation constants, the field
// tangents, the vignetting factors, the centre, where its hits and its eight sums go -- is
// workgroup-uniform and read with scalar loads; no lane knows which variant it traces.
//
// The body is spot_trace_kernel's (trace_kernel.hip, included for its pieces: LanePack, SpotAcc,
// store_plane, the surface walk of surface_math.h): generate -> trace -> reduce, the lean fp32
// form on packed pairs, the Newton family chosen once from the shared structure.  A translation
// unit of its own: the code objects and kernarg layouts of the existing kernels are what they
// were.  Resources and timings: profiles/ensemble.txt (tools/gpu_ensemble.py).
#define OL_TRACE_TU 3   // trace_kernel.hip without its launchers
#include "trace_kernel.hip"

#include <cstdio>
#include <new>
#include <vector>

#include "../../include/optiland_hip.h"
#include "ensemble_device.h"
#include "ensemble_rules.h"
#include "ensemble_store.h"   // struct ol_ensemble
#include "entry_rules.h"
#include "last_error.h"
#include "system_stage.h"
#include "table_image.h"

namespace ol {

template <typename T>
struct EnsembleArgs {
  EnsembleTables<T> tab;
  const ol_ensemble_cell* cells;   // device, [n_cells]
  const T *px, *py;                // the pupil planes every cell traces
  T* hits;                         // nullptr, or cell 0's x plane (cell c: + 3 c hits_stride)
  int64_t hits_stride;
  double* out;                     // [n_cells][8], accumulated
  uint32_t* status;
  int64_t n, n_cells;
  uint32_t flags;                  // OL_RAYGEN_* | OL_SPOT_HITS_LOCAL
  int32_t tiles_per_block;
};

// (namespace ol, not an anonymous one: tools/kernel_resources.py and rocprofv3 name the kernels)
template <typename T, int RPT, int NR, bool APOD>
__global__ __launch_bounds__(kTraceBlock) void ensemble_spot_kernel(EnsembleArgs<T> a) {
  // table rows re-read phase by phase where spot_trace_kernel does so (fetch level 2)
  constexpr bool kFetchRows = fetch_level<T, NR, true>() >= 2;

  const int64_t cell_i = ensemble_cell_index(blockIdx.y, blockIdx.z, gridDim.y);
  if (cell_i >= a.n_cells) return;   // (workgroup-uniform, like every exit below)
  const cptr<ol_ensemble_cell> cell = as_const(a.cells) + cell_i;
  const int32_t variant = cell->variant, wl = cell->wavelength_index;
  if (!ensemble_cell_ok(a.tab, variant, wl)) {
    if (threadIdx.x == 0) atomicOr(a.status, kStatusEnsembleCell);
    return;
  }
  const EnsembleRows<T> rows = ensemble_rows(a.tab, variant, wl);
  const int n_surf = a.tab.n_surf, n_wl = a.tab.n_wl;

  SpotAcc acc;
  uint32_t status = 0;
  const uint32_t rg_flags = a.flags;
  // the cell's field point, once per workgroup (the tangent of an angle field is a double-
  // precision tan(): per tile it would cost what it costs spot_trace_kernel per ray)
  const EnsembleField<T> f = ensemble_field<T>(load_consts(rows.rgc), cell, rg_flags, status);

  constexpr int64_t kTileRays = (int64_t)kTraceBlock * RPT;
  const int64_t ntiles = (a.n + kTileRays - 1) / kTileRays;
  for (int tt = 0; tt < a.tiles_per_block; ++tt) {
    const int64_t tile = (int64_t)blockIdx.x * a.tiles_per_block + tt;
    if (tile >= ntiles) break;
    const int64_t base = (tile * kTraceBlock + threadIdx.x) * RPT;
    const int64_t left = a.n - base;
    const int cnt = left >= RPT ? RPT : (left > 0 ? (int)left : 0);

    // pupil planes; lanes past the end trace the on-axis pupil point and are masked out
    T in[2][RPT];
    if (RPT > 1 && cnt == RPT) {
      using VT = typename VecOf<T, RPT>::type;
      const VT vx_ = *reinterpret_cast<const VT*>(a.px + base);
      const VT vy_ = *reinterpret_cast<const VT*>(a.py + base);
#pragma unroll
      for (int k = 0; k < RPT; ++k) {
        in[0][k] = vec_get<T, RPT>(vx_, k);
        in[1][k] = vec_get<T, RPT>(vy_, k);
      }
    } else {
#pragma unroll
      for (int k = 0; k < RPT; ++k) {
        const bool ok = k < cnt;
        in[0][k] = ok ? a.px[base + k] : T(0);
        in[1][k] = ok ? a.py[base + k] : T(0);
      }
    }

    using LP = LanePack<T, RPT, 0, NR>;  // fp32 lean kernel: packed pairs of rays
    using V = typename LP::V;
    constexpr int NV = LP::NV;
    Ray<V> r[NV];
    {
      // (read again per tile: the constants die with the generator instead of riding the
      // surface loop in scalar registers)
      const RaygenConsts<T> c = load_consts(refresh(rows.rgc));
#pragma unroll
      for (int k = 0; k < RPT; ++k) {
        T o[6];
        T vx = f.vx, vy = f.vy;
        raygen_pupil<T>(rg_flags, vx, vy, in[0][k], in[1][k], status);
        raygen_one<T>(c, f.tx, f.ty, in[0][k], in[1][k], vx, vy, o);
        Ray<T> q;
        q.x = o[0]; q.y = o[1]; q.z = o[2];
        q.L = o[3]; q.M = o[4]; q.N = o[5];
        if constexpr (APOD) q.i = raygen_apodize<T>(c, in[0][k], in[1][k]); else q.i = T(1);
        q.opd = T(0);
        LP::put(r, k, q);
      }
    }

    Ray<V> gv[NV];
    ensemble_walk<T, V, NV, NR, (RPT > 1), kFetchRows>(rows, n_surf, n_wl,
                                                       (rg_flags & kSpotHitsLocal) != 0, r, gv,
                                                       status);

    T hx_[RPT], hy_[RPT], hi_[RPT];
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
      const Ray<T> g = LP::ray(gv, k);
      hx_[k] = g.x; hy_[k] = g.y; hi_[k] = g.i;
      if (k < cnt) acc.add(g.x, g.y, g.i, f.cx, f.cy);
    }
    if (a.hits != nullptr && cnt > 0) {
      const RayIndexT<false> at{tile * (kTraceBlock * RPT), (uint32_t)threadIdx.x * RPT};
      T* plane = a.hits + cell_i * 3 * a.hits_stride;
      store_plane<T, RPT>(plane, at, cnt, hx_);
      store_plane<T, RPT>(plane + a.hits_stride, at, cnt, hy_);
      store_plane<T, RPT>(plane + 2 * a.hits_stride, at, cnt, hi_);
    }
  }

  acc.flush(a.out + 8 * cell_i);
  if (status) atomicOr(a.status, status);
}

namespace {

template <typename T, int RPT, int NR>
hipError_t launch_ensemble_nr(EnsembleArgs<T> a, bool apod, hipStream_t stream) {
  const int64_t tile_rays = (int64_t)kTraceBlock * RPT;
  const int64_t ntiles = (a.n + tile_rays - 1) / tile_rays;
  // as launch_spot_nr: ~8 rounds of resident workgroups over ALL cells, few enough of them per
  // cell that its seven same-address atomics stay far below the L2 atomic rate
  constexpr int64_t kTargetBlocks = 8192;
  int64_t tpb = (ntiles * a.n_cells + kTargetBlocks - 1) / kTargetBlocks;
  if (tpb < 1) tpb = 1;
  if (tpb > 1024) tpb = 1024;
  if (tpb > ntiles) tpb = ntiles;
  a.tiles_per_block = (int32_t)tpb;
  const int64_t blocks = (ntiles + tpb - 1) / tpb;
  if (blocks == 0 || a.n_cells == 0) return hipSuccess;
  if (blocks > 0x7fffffffLL || a.n_cells > kEnsembleMaxCells) return hipErrorInvalidValue;
  uint32_t gy = 1, gz = 1;
  ensemble_grid(a.n_cells, gy, gz);
  const dim3 grid((unsigned)blocks, gy, gz);
  if (apod)
    hipLaunchKernelGGL((ensemble_spot_kernel<T, RPT, NR, true>), grid, dim3(kTraceBlock), 0, stream,
                       a);
  else
    hipLaunchKernelGGL((ensemble_spot_kernel<T, RPT, NR, false>), grid, dim3(kTraceBlock), 0,
                       stream, a);
  return hipGetLastError();
}

// the defaults of dispatch_spot (trace_kernel.hip), so that a variant is traced by the same
// arithmetic as ol_trace_spot traces it alone: conic-only ranges on the 16-byte vector of rays
// per lane, Newton ranges one ray per lane in the family the shared structure allows
template <typename T>
hipError_t launch_ensemble(const EnsembleArgs<T>& a, bool vector_ok, int nr_family, bool apod,
                           hipStream_t stream) {
  constexpr int kVec = 16 / sizeof(T);
  if (nr_family == kNrReference) return hipErrorInvalidValue;
  if (nr_family == kNrZernike) return launch_ensemble_nr<T, 1, kNrZernike>(a, apod, stream);
  if (nr_family == kNrEvenAsphere) return launch_ensemble_nr<T, 1, kNrEvenAsphere>(a, apod, stream);
  if (nr_family != kNrNone) return launch_ensemble_nr<T, 1, kNrGeneric>(a, apod, stream);
  if (!vector_ok || tuning().rays_per_thread == 1)
    return launch_ensemble_nr<T, 1, kNrNone>(a, apod, stream);
  return launch_ensemble_nr<T, kVec, kNrNone>(a, apod, stream);
}

inline size_t round256(size_t v) { return (v + 255u) & ~size_t(255u); }
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <typename T>
void release(EnsembleStore<T>& s) {
  if (s.blob) (void)hipFree(s.blob);
  s = EnsembleStore<T>();
}

RaygenDev raygen_of(const ol_raygen_params& g) {
  return RaygenDev{g.object_infinite, g.field_kind, g.EPL,     g.EPD,    g.max_field,
                   g.offset,          g.z_first,    g.tele_dz, g.apod_a, g.apod_b,
                   g.apod_kind};
}

}  // namespace
}  // namespace ol

using namespace ol;

namespace {

#define OL_HIP_CHECK(who, expr)                                                          \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess)                                                                \
      return failf(OL_EHIP, "%s: %s failed: %s", who, #expr, hipGetErrorString(e_));     \
  } while (0)

// variants[0 .. count) checked and staged as variants k0 ... of an ensemble whose variant 0 is
// (ref_rows, ref_coeffs, ref_raygen, ref); all of them before anything is copied
int stage_variants(const char* who, const ol_ensemble_variant* variants, int32_t k0, int32_t count,
                   int32_t n_surf, int32_t n_wl, const ol_surface_desc* ref_rows,
                   int32_t ref_coeffs, const ol_raygen_params& ref_raygen, const Staged& ref,
                   std::vector<Staged>& out) {
  out.assign(count, Staged());
  for (int32_t i = 0; i < count; ++i) {
    const ol_ensemble_variant& v = variants[i];
    const int32_t k = k0 + i;
    if (int rc = rule_variant_record(who, k, v)) return rc;
    if (int rc = rule_same_rows(who, k, ref_rows, ref_coeffs, v.surf, v.n_coeffs, n_surf)) return rc;
    if (int rc = rule_same_raygen(who, k, ref_raygen, *v.raygen)) return rc;
    char name[64];
    snprintf(name, sizeof(name), "%s: variant %d", who, k);
    if (int rc = stage_system(name, v.surf, n_surf, v.coeffs, v.n_coeffs, v.optics, n_wl, out[i]))
      return rc;
    if (int rc = rule_same_staging(who, k, ref, out[i])) return rc;
  }
  return OL_OK;
}

template <typename T>
void fill_range(const ol_ensemble& e, const std::vector<Staged>& st,
                const ol_ensemble_variant* variants, RangeImage<T>& im) {
  const size_t count = st.size(), ns = (size_t)e.n_surf, no = ns * (size_t)e.n_wl;
  im.surf.assign(count * ns, DevSurfHot<T>());
  im.cold.assign(count * ns, DevSurfCold<T>());
  im.optics.assign(count * no, DevOptics<T>());
  im.coeffs.assign(count * e.coef_cap, T(0));
  im.rgc.assign(count, RaygenConsts<T>());
  for (size_t i = 0; i < count; ++i) {
    write_table_image<T>(st[i].surf, st[i].optics, st[i].coeffs, st[i].int_slots,
                         im.surf.data() + i * ns, im.cold.data() + i * ns,
                         im.optics.data() + i * no, im.coeffs.data() + i * e.coef_cap);
    im.rgc[i] = RaygenConsts<T>(raygen_of(*variants[i].raygen));
  }
}

template <typename T>
int allocate(const ol_ensemble& e, EnsembleStore<T>& s) {
  const size_t K = (size_t)e.n_variants, ns = (size_t)e.n_surf, no = ns * (size_t)e.n_wl;
  const size_t off_cold = round256(K * ns * sizeof(DevSurfHot<T>));
  const size_t off_opt = off_cold + round256(K * ns * sizeof(DevSurfCold<T>));
  const size_t off_coef = off_opt + round256(K * no * sizeof(DevOptics<T>));
  const size_t off_rgc = off_coef + round256(K * e.coef_cap * sizeof(T));
  const size_t bytes = off_rgc + K * sizeof(RaygenConsts<T>);
  OL_HIP_CHECK("ol_ensemble_create", hipMalloc((void**)&s.blob, bytes));
  s.dev.surf = reinterpret_cast<DevSurfHot<T>*>(s.blob);
  s.dev.cold = reinterpret_cast<DevSurfCold<T>*>(s.blob + off_cold);
  s.dev.optics = reinterpret_cast<DevOptics<T>*>(s.blob + off_opt);
  s.dev.coeffs = reinterpret_cast<T*>(s.blob + off_coef);
  s.dev.rgc = reinterpret_cast<RaygenConsts<T>*>(s.blob + off_rgc);
  s.dev.n_variants = e.n_variants;
  s.dev.n_surf = e.n_surf;
  s.dev.n_wl = e.n_wl;
  s.dev.coef_cap = (int32_t)e.coef_cap;
  return OL_OK;
}

// variants [k0, k0 + count) of every table: five copies out of `im` (which the caller keeps until
// the copies are known to be done), queued on `stream`
template <typename T>
int upload(const char* who, const ol_ensemble& e, const EnsembleStore<T>& s, int32_t k0,
           const std::vector<Staged>& st, const ol_ensemble_variant* variants, RangeImage<T>& im,
           hipStream_t stream) {
  fill_range<T>(e, st, variants, im);
  const size_t ns = (size_t)e.n_surf, no = ns * (size_t)e.n_wl, k = (size_t)k0;
  auto copy = [&](const void* dst, const auto& v) {
    return hipMemcpyAsync(const_cast<void*>(dst), v.data(), v.size() * sizeof(v[0]),
                          hipMemcpyHostToDevice, stream);
  };
  OL_HIP_CHECK(who, copy(s.dev.surf + k * ns, im.surf));
  OL_HIP_CHECK(who, copy(s.dev.cold + k * ns, im.cold));
  OL_HIP_CHECK(who, copy(s.dev.optics + k * no, im.optics));
  OL_HIP_CHECK(who, copy(s.dev.coeffs + k * e.coef_cap, im.coeffs));
  OL_HIP_CHECK(who, copy(s.dev.rgc + k, im.rgc));
  return OL_OK;
}

template <typename T>
int do_trace_spot_ensemble(const ol_ensemble* ens, const EnsembleStore<T>& s, int64_t n,
                           const ol_raygen_inputs* in, int64_t n_cells,
                           const ol_ensemble_cell* cells_dev, void* hits, int64_t hits_stride,
                           double* out8, uint32_t* status, hipStream_t stream) {
  EnsembleArgs<T> a{};
  a.tab = s.dev;
  a.cells = cells_dev;
  a.px = static_cast<const T*>(in->px);
  a.py = static_cast<const T*>(in->py);
  a.hits = static_cast<T*>(hits);
  a.hits_stride = hits_stride;
  a.out = out8;
  a.status = status;
  a.n = n;
  a.n_cells = n_cells;
  a.flags = in->flags;
  a.tiles_per_block = 1;
  // every cell's planes must keep the 16-byte alignment the vector accesses need
  const bool vec = aligned16(in->px) && aligned16(in->py) && aligned16(hits) &&
                   (hits_stride * (int64_t)sizeof(T)) % 16 == 0;
  const hipError_t e = launch_ensemble<T>(a, vec, ens->family, ens->apod, stream);
  if (e != hipSuccess)
    return failf(OL_EHIP, "ol_trace_spot_ensemble: launch failed: %s", hipGetErrorString(e));
  return OL_OK;
}

}  // namespace

extern "C" {

int ol_ensemble_create(const ol_ensemble_variant* variants, int32_t n_variants, int32_t n_surf,
                       int32_t n_wavelengths, ol_ensemble** out) {
  const char* who = "ol_ensemble_create";
  if (!out) return failf(OL_EINVAL, "%s: out is NULL", who);
  *out = nullptr;
  if (!variants || n_variants <= 0) return failf(OL_EINVAL, "%s: no variants", who);
  if (int rc = rule_variant_record(who, 0, variants[0])) return rc;
  ol_ensemble* e = new (std::nothrow) ol_ensemble();
  if (!e) return failf(OL_ENOMEM, "%s: out of host memory", who);
  struct Guard {
    ol_ensemble* e;
    ~Guard() { if (e) ol_ensemble_destroy(e); }
  } guard{e};
  e->n_variants = n_variants;
  e->n_surf = n_surf;
  e->n_wl = n_wavelengths;
  // variant 0 first: it is the structure, and what the launch could not serve is refused on it
  const ol_ensemble_variant& v0 = variants[0];
  if (int rc = stage_system("ol_ensemble_create: variant 0", v0.surf, n_surf, v0.coeffs,
                            v0.n_coeffs, v0.optics, n_wavelengths, e->ref))
    return rc;
  if (int rc = rule_no_reference_newton(who, facts_view(e->ref.facts, n_surf, n_wavelengths, 0)))
    return rc;
  e->ref_rows.assign(v0.surf, v0.surf + n_surf);
  e->ref_coeffs = v0.n_coeffs;
  e->ref_raygen = *v0.raygen;
  e->coef_cap = e->ref.coeffs.size() ? e->ref.coeffs.size() : 1;
  e->family = newton_family_of(e->ref.facts, 0, n_surf - 1);
  e->apod = v0.raygen->apod_kind != 0;
  std::vector<Staged> st;   // (variant 0 is staged: the others, then its image in front of them)
  if (int rc = stage_variants(who, variants + 1, 1, n_variants - 1, n_surf, n_wavelengths,
                              e->ref_rows.data(), e->ref_coeffs, e->ref_raygen, e->ref, st))
    return rc;
  st.insert(st.begin(), e->ref);
  if (!current_device(&e->device))
    return failf(OL_EHIP, "%s: no HIP device (hipGetDevice failed)", who);
  if (int rc = allocate<float>(*e, e->f32)) return rc;
  if (int rc = allocate<double>(*e, e->f64)) return rc;
  OL_HIP_CHECK(who, hipEventCreateWithFlags(&e->copied, hipEventDisableTiming));
  if (int rc = upload<float>(who, *e, e->f32, 0, st, variants, e->image32, nullptr)) return rc;
  if (int rc = upload<double>(who, *e, e->f64, 0, st, variants, e->image64, nullptr)) return rc;
  OL_HIP_CHECK(who, hipStreamSynchronize(nullptr));
  e->image32 = RangeImage<float>();    // (the copies are done: the whole-ensemble images may go)
  e->image64 = RangeImage<double>();
  guard.e = nullptr;
  *out = e;
  return OL_OK;
}

int ol_ensemble_update(ol_ensemble* ens, int32_t k0, int32_t count,
                       const ol_ensemble_variant* variants, void* stream) {
  const char* who = "ol_ensemble_update";
  if (int rc = rule_ensemble(who, ens)) return rc;
  if (int rc = rule_variant_range(who, k0, count, ens->n_variants)) return rc;
  if (count == 0) return OL_OK;
  if (!variants) return failf(OL_EINVAL, "%s: variants is NULL", who);
  std::vector<Staged> st;
  if (int rc = stage_variants(who, variants, k0, count, ens->n_surf, ens->n_wl,
                              ens->ref_rows.data(), ens->ref_coeffs, ens->ref_raygen, ens->ref,
                              st))
    return rc;
  if (int rc = rule_consistent(who, ens->consistent)) return rc;
  if (int rc = rule_current_device(
          who, facts_view(ens->ref.facts, ens->n_surf, ens->n_wl, ens->device)))
    return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // the previous update's copies read the images this one is about to write
  OL_HIP_CHECK(who, hipEventSynchronize(ens->copied));
  // fp64 first, as ol_system_update: if its copies fail before any was queued nothing has changed
  if (int rc = upload<double>(who, *ens, ens->f64, k0, st, variants, ens->image64, s)) return rc;
  ens->consistent = false;
  if (int rc = upload<float>(who, *ens, ens->f32, k0, st, variants, ens->image32, s)) return rc;
  OL_HIP_CHECK(who, hipEventRecord(ens->copied, s));
  ens->consistent = true;
  return OL_OK;
}

void ol_ensemble_destroy(ol_ensemble* ens) {
  if (!ens) return;
  if (ens->copied) {
    (void)hipEventSynchronize(ens->copied);   // (a queued copy may still read the images)
    (void)hipEventDestroy(ens->copied);
  }
  release(ens->f32);
  release(ens->f64);
  delete ens;
}

int32_t ol_ensemble_size(const ol_ensemble* ens) { return ens ? ens->n_variants : 0; }

int ol_trace_spot_ensemble(const ol_ensemble* ens, ol_dtype dt, int64_t n_rays,
                           const ol_raygen_inputs* in, int64_t n_cells,
                           const ol_ensemble_cell* cells_dev, void* hits, int64_t hits_stride,
                           double* out8, uint32_t* status, void* stream) {
  const char* who = "ol_trace_spot_ensemble";
  if (int rc = rule_ensemble(who, ens)) return rc;
  if (int rc = rule_consistent(who, ens->consistent)) return rc;
  if (int rc = rule_dtype(who, dt)) return rc;
  if (!in || !in->px || !in->py || !out8 || !status || (n_cells > 0 && !cells_dev))
    return failf(OL_EINVAL, "%s: NULL argument", who);
  if (int rc = rule_count(who, n_rays, "negative ray count")) return rc;
  if (n_cells < 0 || n_cells > kEnsembleMaxCells)
    return failf(OL_EINVAL, "%s: %lld cells outside [0, %lld]", who, (long long)n_cells,
                 (long long)kEnsembleMaxCells);
  if (in->hx || in->hy || in->vx || in->vy)
    return failf(OL_EINVAL, "%s: per-ray field / vignetting planes with cells (each cell has ONE "
                            "field point)", who);
  if (hits && hits_stride < n_rays)
    return failf(OL_EINVAL, "%s: hits_stride %lld < %lld rays", who, (long long)hits_stride,
                 (long long)n_rays);
  const SystemView v = facts_view(ens->ref.facts, ens->n_surf, ens->n_wl, ens->device);
  if (!(in->flags & OL_SPOT_POLARIZED_OK))
    if (int rc = rule_polarisation_required(v, 0, v.n_surf - 1)) return rc;
  if (n_rays == 0 || n_cells == 0) return OL_OK;
  if (int rc = rule_current_device(who, v)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dt == OL_F32)
    return do_trace_spot_ensemble<float>(ens, ens->f32, n_rays, in, n_cells, cells_dev, hits,
                                         hits_stride, out8, status, st);
  return do_trace_spot_ensemble<double>(ens, ens->f64, n_rays, in, n_cells, cells_dev, hits,
                                        hits_stride, out8, status, st);
}

}  // extern "C"
