// ensemble_opd.hip -- the OPD maps of K variants of one optic in ONE call (ol_trace_opd_ensemble).
//
// Reference: optimization/operand/ray.py:343-389 (OPD_difference) -- per tolerancing iteration a
// Wavefront at one field and wavelength, reduced to a mean absolute deviation.  Through an
// ol_system that is, per variant, one table upload, one chief-ray launch (ol_wavefront_reference),
// one OPD launch of a few hundred rays (ol_trace_opd_dev) and one read-back.  Here the variants
// are an ol_ensemble's (ensemble.hip) and two launches serve every (variant, field, wavelength)
// cell:
//   ensemble_chief_kernel   one workgroup per cell, one lane: the cell's chief ray -> its
//                           reference sphere / plane, left in the cell's slot of `refs`
//   ensemble_opd_kernel     blockIdx.x a block of ray tiles, the cell from blockIdx.y / .z as in
//                           ensemble_spot_kernel: generate -> walk -> OPD against the cell's slot
//                           -> the twelve moments, added into the cell's own
// Everything a cell selects is workgroup-uniform and read with scalar loads
// (ensemble_opd_device.h); no lane knows its variant.  One ray per lane always: a cell is a few
// hundred rays, and the two-ray form of opd_trace_kernel only starts at 4096 workgroups of ONE
// cell.  A translation unit of its own: the code objects and kernarg layouts of the existing
// kernels are what they were.  Resources and timings: profiles/ensemble_opd.txt
// (tools/gpu_ensemble_opd.py).
#define OL_TRACE_TU 3   // trace_kernel.hip without its launchers
#include "trace_kernel.hip"

#include "../../include/optiland_hip.h"
#include "ensemble_device.h"
#include "ensemble_opd_device.h"
#include "ensemble_rules.h"
#include "ensemble_store.h"   // struct ol_ensemble
#include "entry_rules.h"
#include "last_error.h"

namespace ol {

constexpr int kOpdPlanes = 2, kOpdPlanesPupil = 5;   // OPD, intensity (+ the pupil point)
static_assert(sizeof(WavefrontConsts<double>) <= OL_WAVEFRONT_REFERENCE_DOUBLES * sizeof(double),
              "header: the device reference structure");

struct EnsembleOpdArgs {
  EnsembleTables<double> tab;
  const ol_ensemble_opd_cell* cells;   // device, [n_cells]
  const double *px, *py;               // the pupil planes every cell traces
  double* refs;                        // [n_cells][OL_WAVEFRONT_REFERENCE_DOUBLES]
  double* planes;                      // nullptr, or cell 0's OPD plane (cell c: + P c stride)
  int64_t planes_stride;
  double* mom;                         // [n_cells][kOpdMoments], accumulated
  uint32_t* status;
  int64_t n, n_cells;
  uint32_t flags;                      // OL_RAYGEN_* | OL_OPD_ENSEMBLE_PUPIL
  int32_t tiles_per_block;
};

constexpr uint32_t kOpdEnsemblePupil = OL_OPD_ENSEMBLE_PUPIL;

OL_DEV WavefrontConsts<double>* ref_slot(double* refs, int64_t cell_i) {
  return reinterpret_cast<WavefrontConsts<double>*>(refs +
                                                    cell_i * OL_WAVEFRONT_REFERENCE_DOUBLES);
}

// (namespace ol, not an anonymous one: tools/kernel_resources.py and rocprofv3 name the kernels)
template <int NR>
__global__ __launch_bounds__(64) void ensemble_chief_kernel(EnsembleOpdArgs a) {
  const int64_t cell_i = ensemble_cell_index(blockIdx.y, blockIdx.z, gridDim.y);
  if (cell_i >= a.n_cells) return;   // (workgroup-uniform)
  if (threadIdx.x != 0) return;      // a cold kernel: one lane per cell
  const cptr<ol_ensemble_opd_cell> cell = as_const(a.cells) + cell_i;
  const int32_t variant = cell->variant, wl = cell->wavelength_index;
  if (!ensemble_cell_ok(a.tab, variant, wl)) {
    atomicOr(a.status, kStatusEnsembleCell);
    return;
  }
  const EnsembleRows<double> rows = ensemble_rows(a.tab, variant, wl);
  uint32_t status = 0;
  *ref_slot(a.refs, cell_i) =
      opd_cell_chief<NR>(rows, a.tab.n_surf, a.tab.n_wl, cell, a.flags, status);
  if (status) atomicOr(a.status, status);
}

template <int NR, bool APOD>
__global__ __launch_bounds__(kTraceBlock) void ensemble_opd_kernel(EnsembleOpdArgs a) {
  // table rows re-read phase by phase where opd_trace_kernel does so (fetch level 2)
  constexpr bool kFetchRows = fetch_level<double, NR, true>() >= 2;

  const int64_t cell_i = ensemble_cell_index(blockIdx.y, blockIdx.z, gridDim.y);
  if (cell_i >= a.n_cells) return;   // (workgroup-uniform, like every exit below)
  const cptr<ol_ensemble_opd_cell> cell = as_const(a.cells) + cell_i;
  const int32_t variant = cell->variant, wl = cell->wavelength_index;
  if (!ensemble_cell_ok(a.tab, variant, wl)) {
    if (threadIdx.x == 0) atomicOr(a.status, kStatusEnsembleCell);
    return;
  }
  const EnsembleRows<double> rows = ensemble_rows(a.tab, variant, wl);
  const int n_surf = a.tab.n_surf, n_wl = a.tab.n_wl;
  const cptr<WavefrontConsts<double>> ref = as_const(ref_slot(a.refs, cell_i));

  uint32_t status = 0;
  const uint32_t rg_flags = a.flags;
  // the cell's field point, once per workgroup (the tangent of an angle field is a double-
  // precision tan())
  const OpdCellField f = opd_cell_field(load_consts(rows.rgc), cell, rg_flags, status);
  double s[kOpdMoments];
#pragma unroll
  for (int k = 0; k < kOpdMoments; ++k) s[k] = 0.0;

  const int64_t ntiles = (a.n + kTraceBlock - 1) / kTraceBlock;
  for (int tt = 0; tt < a.tiles_per_block; ++tt) {
    const int64_t tile = (int64_t)blockIdx.x * a.tiles_per_block + tt;
    if (tile >= ntiles) break;
    const int64_t j = tile * kTraceBlock + threadIdx.x;
    if (j < a.n) {
      double ov, gi, pu[3];
      opd_cell_trace<NR, APOD, kFetchRows>(rows, n_surf, n_wl, f, rg_flags, ref, a.px[j], a.py[j],
                                           status, ov, gi, pu);
      if (a.planes != nullptr) {
        const bool pupil = (rg_flags & kOpdEnsemblePupil) != 0;
        double* plane =
            a.planes + cell_i * (pupil ? kOpdPlanesPupil : kOpdPlanes) * a.planes_stride + j;
        plane[0] = ov;
        plane[a.planes_stride] = gi;
        if (pupil) {
          plane[2 * a.planes_stride] = pu[0];
          plane[3 * a.planes_stride] = pu[1];
          plane[4 * a.planes_stride] = pu[2];
        }
      }
      opd_accumulate(s, gi, ov, pu[0], pu[1], gi > 0.0);
    }
  }

  // workgroup reduction -> kOpdMoments atomics (every thread of a traced cell reaches this point)
  __shared__ double part[kTraceBlock / 64][kOpdMoments];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    double t[kOpdMoments];
#pragma unroll
    for (int k = 0; k < kOpdMoments; ++k) t[k] = __shfl_down(s[k], off, 64);
#pragma unroll
    for (int k = 0; k < kOpdMoments; ++k) s[k] += t[k];
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kOpdMoments; ++k) part[wave][k] = s[k];
  }
  __syncthreads();
  if (threadIdx.x < kOpdMoments) {
    double v = 0;
    for (int q = 0; q < kTraceBlock / 64; ++q) v += part[q][threadIdx.x];
    // (a NaN partial sum must reach the output too: v != 0.0 is true for NaN)
    if (v != 0.0) unsafeAtomicAdd(a.mom + kOpdMoments * cell_i + threadIdx.x, v);
  }
  if (status) atomicOr(a.status, status);
}

namespace {

template <int NR>
hipError_t launch_ensemble_opd_nr(EnsembleOpdArgs a, bool apod, hipStream_t stream) {
  uint32_t gy = 1, gz = 1;
  ensemble_grid(a.n_cells, gy, gz);
  // the chief rays first: the OPD launch reads what they leave, in stream order.  (cold: the
  // generic Newton instantiation serves every family, as in launch_chief_reference)
  if (NR == kNrNone)
    hipLaunchKernelGGL((ensemble_chief_kernel<kNrNone>), dim3(1, gy, gz), dim3(64), 0, stream, a);
  else
    hipLaunchKernelGGL((ensemble_chief_kernel<kNrGeneric>), dim3(1, gy, gz), dim3(64), 0, stream,
                       a);
  if (hipError_t e = hipGetLastError()) return e;

  const int64_t ntiles = (a.n + kTraceBlock - 1) / kTraceBlock;
  // as launch_ensemble_nr: ~8 rounds of resident workgroups over ALL cells, few enough of them per
  // cell that its twelve same-address atomics stay far below the L2 atomic rate
  constexpr int64_t kTargetBlocks = 8192;
  int64_t tpb = (ntiles * a.n_cells + kTargetBlocks - 1) / kTargetBlocks;
  if (tpb < 1) tpb = 1;
  if (tpb > 1024) tpb = 1024;
  if (tpb > ntiles) tpb = ntiles;
  a.tiles_per_block = (int32_t)tpb;
  const int64_t blocks = (ntiles + tpb - 1) / tpb;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks, gy, gz);
  if (apod)
    hipLaunchKernelGGL((ensemble_opd_kernel<NR, true>), grid, dim3(kTraceBlock), 0, stream, a);
  else
    hipLaunchKernelGGL((ensemble_opd_kernel<NR, false>), grid, dim3(kTraceBlock), 0, stream, a);
  return hipGetLastError();
}

// the Newton family of opd_trace_kernel for the shared structure, so that a variant's map is the
// arithmetic of ol_trace_opd_dev on that variant alone
hipError_t launch_ensemble_opd(const EnsembleOpdArgs& a, int nr_family, bool apod,
                               hipStream_t stream) {
  if (nr_family == kNrReference) return hipErrorInvalidValue;
  if (nr_family == kNrZernike) return launch_ensemble_opd_nr<kNrZernike>(a, apod, stream);
  if (nr_family == kNrEvenAsphere) return launch_ensemble_opd_nr<kNrEvenAsphere>(a, apod, stream);
  if (nr_family != kNrNone) return launch_ensemble_opd_nr<kNrGeneric>(a, apod, stream);
  return launch_ensemble_opd_nr<kNrNone>(a, apod, stream);
}

}  // namespace
}  // namespace ol

using namespace ol;

extern "C" int ol_trace_opd_ensemble(const ol_ensemble* ens, ol_dtype dt, int64_t n_rays,
                                     const ol_raygen_inputs* in, int64_t n_cells,
                                     const ol_ensemble_opd_cell* cells_dev, void* refs,
                                     void* planes, int64_t planes_stride, double* moments12,
                                     uint32_t* status, void* stream) {
  const char* who = "ol_trace_opd_ensemble";
  if (int rc = rule_ensemble(who, ens)) return rc;
  if (int rc = rule_consistent(who, ens->consistent)) return rc;
  if (int rc = rule_fp64_only(who, dt)) return rc;
  if (!in || !in->px || !in->py || !refs || !moments12 || !status || (n_cells > 0 && !cells_dev))
    return failf(OL_EINVAL, "%s: NULL argument", who);
  if (int rc = rule_count(who, n_rays, "negative ray count")) return rc;
  if (n_cells < 0 || n_cells > kEnsembleMaxCells)
    return failf(OL_EINVAL, "%s: %lld cells outside [0, %lld]", who, (long long)n_cells,
                 (long long)kEnsembleMaxCells);
  if (in->hx || in->hy || in->vx || in->vy)
    return failf(OL_EINVAL, "%s: per-ray field / vignetting planes with cells (each cell has ONE "
                            "field point)", who);
  if (planes && planes_stride < n_rays)
    return failf(OL_EINVAL, "%s: planes_stride %lld < %lld rays", who, (long long)planes_stride,
                 (long long)n_rays);
  const SystemView v = facts_view(ens->ref.facts, ens->n_surf, ens->n_wl, ens->device);
  if (int rc = rule_no_reference_newton(who, v)) return rc;
  if (int rc = rule_polarisation_required(v, 0, v.n_surf - 1)) return rc;
  if (n_rays == 0 || n_cells == 0) return OL_OK;
  if (int rc = rule_current_device(who, v)) return rc;

  EnsembleOpdArgs a{};
  a.tab = ens->f64.dev;
  a.cells = cells_dev;
  a.px = static_cast<const double*>(in->px);
  a.py = static_cast<const double*>(in->py);
  a.refs = static_cast<double*>(refs);
  a.planes = static_cast<double*>(planes);
  a.planes_stride = planes_stride;
  a.mom = moments12;
  a.status = status;
  a.n = n_rays;
  a.n_cells = n_cells;
  a.flags = in->flags;
  a.tiles_per_block = 1;
  const hipError_t e =
      launch_ensemble_opd(a, ens->family, ens->apod, static_cast<hipStream_t>(stream));
  if (e != hipSuccess)
    return failf(OL_EHIP, "%s: launch failed: %s", who, hipGetErrorString(e));
  return OL_OK;
}
