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
// rule_no_single_kinds).
//
// Shape of the launch: single_surface.h, shared with forbes.hip.
// 8 planes read, up to 16 written.  The
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
#include "single_surface.h"

// (namespace ol, not an anonymous one: tools/asm_stats.py and rocprofv3 name the kernels)
namespace ol {

template <typename T>
__global__ __launch_bounds__(kSingleThreads) void grid_sag_trace_kernel(SingleArgs<T> a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;   // (the Newton loop's vote is among the lanes that stay)
  const Ray<T> r = single_load(a, i);
  const Ray<T> g = grid_sag_step<T>(single_fetched(a), as_const(a.coeffs), a.coeffs, r);
  single_store(a, i, g);
  // a ray without a direction: total internal reflection, or a ray that left the grid (whose
  // position is NaN as well; see OL_STATUS_NAN_DIRECTION).  One lane per wave writes: a bundle
  // wider than its grid has NaN rays by the million, and they would all meet at the one word
  if (a.status != nullptr && !(a.flags & OL_TRACE_MIDRANGE)) {
    if (hw::wave_any(g.L != g.L) && hw::wave_leader()) atomicOr(a.status, kStatusNanDirection);
  }
}

}  // namespace ol

using namespace ol;

extern "C" int ol_trace_grid_sag(const ol_system* sys, ol_dtype dt, int64_t n_rays,
                                 void* const rays[8], int32_t wavelength_index, void* record_row,
                                 int64_t record_stride, int32_t surface, uint32_t flags,
                                 uint32_t* status, void* stream) {
  if (int rc = grid_sag_check(sys, dt, n_rays, rays, wavelength_index, record_row,
                              record_stride, surface, flags))
    return rc;
  return single_entry(kSingleKinds[kSingleGridSag].entry, sys, dt, n_rays, stream,
                      [&](auto t, const SystemView& v, hipStream_t st) {
    using T = decltype(t);
    const SingleArgs<T> a = single_args<T>(v, surface, wavelength_index, n_rays, rays, record_row,
                                           record_stride, flags, status);
    const SingleGrid g = single_grid(n_rays);
    hipLaunchKernelGGL((grid_sag_trace_kernel<T>), g.blocks, g.threads, 0, st, a);
  });
}
