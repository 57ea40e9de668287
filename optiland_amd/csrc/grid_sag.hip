// grid_sag.hip -- one grid-sag surface on the device (ol_trace_grid_sag).
//
// Reference: Surface.trace on GridSagGeometry (surfaces/standard_surface.py:232-274,
// geometries/grid_sag.py): a Python Newton loop of up to max_iter = 100 passes, each with two
// searchsorted, eight fancy-index gathers, some forty elementwise operations and a host
// synchronisation at `be.max(be.abs(dt)) < tol`; one ray that leaves the grid turns NaN, makes
// that test false and has the whole bundle run all 100 passes.  Here the surface is ONE launch
// between two fused runs of ol_trace: one ray per lane, the frame change, the solve stopped per
// ray (grid_sag_device.h), the interaction (surface_math.h: interact<>, as the fused kernels use
// it), the way back to the global frame and the stores of the ray state and of the recorded row.
// Nothing is shared between lanes but the OR of the status word.  The fused kernels do not know
// these surfaces: their entry points refuse a range that holds one (entry_rules.h:
// rule_no_grid_sag).
//
// Shape of the launch: that of forbes_launch (forbes.hip).  8 planes read, up to 16 written.  The
// head of the block is wave-uniform scalar loads; the two coordinate pairs and the four nodes of
// a cell are per-lane loads, every index clamped before the load (grid_sag_device.h).  The
// Newton loop's trip count differs per lane (2-5 passes) and each pass has dependent gathers --
// coordinates, then nodes -- so the loop is latency-bound per wave and leans on occupancy: the
// cell indices travel in two registers, nothing is indexed at run time but global memory.
// Compiled for gfx950 (tools/kernel_resources.py on the object):
//   grid_sag_trace_kernel<float>    60 VGPRs, 78 SGPRs, 8 waves per SIMD
//   grid_sag_trace_kernel<double>   83 VGPRs, 68 SGPRs, 5 waves per SIMD
// no scratch, no LDS, no spills.  Measured on the MI355X: profiles/grid_sag.txt
// (tools/gpu_grid_sag.py) -- launch-bound up to 1e5 rays; at 1e7 rays 4.0 / 4.8 TB/s of the 24
// planes on the 33 x 29 grid (1.53 / 1.24 of the one-surface even-asphere launch: the dependent
// loads bind, not the planes) and 1.8 / 2.7 TB/s on a 512 x 512 grid (its gathers bind).
#include <hip/hip_runtime.h>

#include "../../include/optiland_hip.h"
#include "grid_sag_device.h"
#include "grid_sag_host.h"
#include "trace_launch.h"

// (namespace ol, not an anonymous one: tools/asm_stats.py and rocprofv3 name the kernels)
namespace ol {

constexpr int kGridSagThreads = 256;

template <typename T>
struct GridSagArgs {
  const DevSurfHot<T>* hot;     // THE surface's rows
  const DevSurfCold<T>* cold;
  const DevOptics<T>* opt;      // its row at the traced wavelength
  const T* coeffs;              // the table's coefficient buffer
  T* rays[8];
  T* row;                       // NULL: nothing recorded
  int64_t stride, n;
  uint32_t* status;
  uint32_t flags;
};

template <typename T>
__global__ __launch_bounds__(kGridSagThreads) void grid_sag_trace_kernel(GridSagArgs<T> a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;   // (the Newton loop's vote is among the lanes that stay)
  Ray<T> r;
  r.x = a.rays[0][i]; r.y = a.rays[1][i]; r.z = a.rays[2][i];
  r.L = a.rays[3][i]; r.M = a.rays[4][i]; r.N = a.rays[5][i];
  r.i = a.rays[6][i]; r.opd = a.rays[7][i];
  const SurfFetched<T> h{as_const(a.hot), as_const(a.cold), as_const(a.opt)};
  const Ray<T> g = grid_sag_step<T>(h, as_const(a.coeffs), a.coeffs, r);
  if (a.row != nullptr) {
    T* p = a.row + i;
    p[0] = g.x; p[a.stride] = g.y; p[2 * a.stride] = g.z;
    p[3 * a.stride] = g.L; p[4 * a.stride] = g.M; p[5 * a.stride] = g.N;
    p[6 * a.stride] = g.i; p[7 * a.stride] = g.opd;
  }
  if (a.flags & kTraceWriteRays) {
    a.rays[0][i] = g.x; a.rays[1][i] = g.y; a.rays[2][i] = g.z;
    a.rays[3][i] = g.L; a.rays[4][i] = g.M; a.rays[5][i] = g.N;
    a.rays[6][i] = g.i; a.rays[7][i] = g.opd;
  }
  // a ray without a direction: total internal reflection, or a ray that left the grid (whose
  // position is NaN as well; see OL_STATUS_NAN_DIRECTION).  One lane per wave writes: a bundle
  // wider than its grid has NaN rays by the million, and they would all meet at the one word
  if (a.status != nullptr && !(a.flags & OL_TRACE_MIDRANGE)) {
    if (hw::wave_any(g.L != g.L) && hw::wave_leader()) atomicOr(a.status, kStatusNanDirection);
  }
}

template <typename T>
void grid_sag_launch(const DevSurfHot<T>* hot, const DevSurfCold<T>* cold,
                     const DevOptics<T>* opt, const T* coeffs, int32_t surface, int32_t n_wl,
                     int32_t wl, int64_t n, void* const rays[8], void* row, int64_t stride,
                     uint32_t flags, uint32_t* status, hipStream_t st) {
  GridSagArgs<T> a{};
  a.hot = hot + surface;
  a.cold = cold + surface;
  a.opt = opt + ((int64_t)surface * n_wl + wl);
  a.coeffs = coeffs;
  for (int k = 0; k < 8; ++k) a.rays[k] = static_cast<T*>(rays[k]);
  a.row = static_cast<T*>(row);
  a.stride = stride;
  a.n = n;
  a.status = status;
  a.flags = flags;
  // small calls: one wave per workgroup, so that the rays spread over the compute units
  const int block = n >= (int64_t)kGridSagThreads * 256 ? kGridSagThreads : 64;
  const unsigned blocks = (unsigned)((n + block - 1) / block);
  hipLaunchKernelGGL((grid_sag_trace_kernel<T>), dim3(blocks), dim3(block), 0, st, a);
}

}  // namespace ol

using namespace ol;

extern "C" int ol_trace_grid_sag(const ol_system* sys, ol_dtype dt, int64_t n_rays,
                                 void* const rays[8], int32_t wavelength_index, void* record_row,
                                 int64_t record_stride, int32_t surface, uint32_t flags,
                                 uint32_t* status, void* stream) {
  if (int rc = grid_sag_check(sys, dt, n_rays, rays, wavelength_index, record_row, record_stride,
                              surface, flags))
    return rc;
  if (n_rays == 0) return OL_OK;
  const SystemView v = system_view(sys);
  if (int rc = rule_current_device("ol_trace_grid_sag", v)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (dt == OL_F32)
    grid_sag_launch<float>(v.surf32, v.cold32, v.optics32, v.coeffs32, surface, v.n_wl,
                           wavelength_index, n_rays, rays, record_row, record_stride, flags,
                           status, st);
  else
    grid_sag_launch<double>(v.surf, v.cold, v.optics, v.coeffs, surface, v.n_wl,
                            wavelength_index, n_rays, rays, record_row, record_stride, flags,
                            status, st);
  Workspace ws{"ol_trace_grid_sag", st};
  return ws.finish();
}
