// forbes.hip -- one Forbes surface on the device (ol_trace_forbes).
//
// Reference: Surface.trace on ForbesQNormalSlopeGeometry / ForbesQ2dGeometry
// (surfaces/standard_surface.py:232-274, geometries/forbes/geometry.py, geometries/forbes/qpoly.py,
// geometries/newton_raphson.py:119-168): per Newton iteration a Python Clenshaw loop per term list
// and derivative order -- hundreds of small array operations on a device backend -- and a host
// synchronisation at the stop test `be.max(be.abs(f_t)) < tol`.  Here the surface is ONE launch
// between two fused runs of ol_trace: one ray per lane, the frame change, the Newton solve
// (forbes_device.h: the sweeps in running registers, stopped per ray), the interaction
// (surface_math.h: interact<>, as the fused kernels use it), the way back to the global frame and
// the stores of the ray state and of the recorded row.  Nothing is shared between lanes but the
// OR of the status word.  The fused kernels do not know these surfaces: their entry points refuse
// a range that holds one (entry_rules.h: rule_no_single_kinds).
//
// Shape of the launch, of this kernel and of its three siblings (grating.hip, phase.hip,
// grid_sag.hip): the arguments, the ray I/O of a lane, the launch shape and the entry's tail are
// stated once, in single_surface.h.
// 8 planes read, up to 16 written, per ray some hundred fp operations per
// Newton iteration: at millions of rays the launch is bound by memory, at the thousands of rays of
// an Optic.trace by launch latency.  The table rows are re-read phase by phase (SurfFetched), so
// no surface field is held in SGPRs across the Newton loop; coefficient reads are wave-uniform
// scalar loads.  One kernel per precision serves both geometries (a wave-uniform branch per
// evaluation).  Compiled for gfx950 (tools/kernel_resources.py on the object):
//   forbes_trace_kernel<float>    84 VGPRs, 78 SGPRs
//   forbes_trace_kernel<double>  144 VGPRs, 82 SGPRs
// no scratch, no LDS, no spills.  Measured on the MI355X: profiles/forbes.txt (tools/gpu_forbes.py).
#include <hip/hip_runtime.h>

#include "../../include/optiland_hip.h"
#include "forbes_device.h"
#include "forbes_host.h"
#include "single_surface.h"

// (namespace ol, not an anonymous one: tools/asm_stats.py and rocprofv3 name the kernels)
namespace ol {

template <typename T>
__global__ __launch_bounds__(kSingleThreads) void forbes_trace_kernel(SingleArgs<T> a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;   // (the Newton loop's vote is among the lanes that stay)
  const Ray<T> r = single_load(a, i);
  const Ray<T> g = forbes_step<T>(single_fetched(a), as_const(a.coeffs), r);
  single_store(a, i, g);
  // total internal reflection: a position without a direction (see OL_STATUS_NAN_DIRECTION)
  const bool report = a.status != nullptr && !(a.flags & OL_TRACE_MIDRANGE);   // (wave-uniform)
  if (report && g.L != g.L && g.x == g.x) atomicOr(a.status, kStatusNanDirection);
}

}  // namespace ol

using namespace ol;

extern "C" int ol_trace_forbes(const ol_system* sys, ol_dtype dt, int64_t n_rays,
                               void* const rays[8], int32_t wavelength_index, void* record_row,
                               int64_t record_stride, int32_t surface, uint32_t flags,
                               uint32_t* status, void* stream) {
  if (int rc = forbes_check(sys, dt, n_rays, rays, wavelength_index, record_row,
                            record_stride, surface, flags))
    return rc;
  return single_entry(kSingleKinds[kSingleForbes].entry, sys, dt, n_rays, stream,
                      [&](auto t, const SystemView& v, hipStream_t st) {
    using T = decltype(t);
    const SingleArgs<T> a = single_args<T>(v, surface, wavelength_index, n_rays, rays, record_row,
                                           record_stride, flags, status);
    const SingleGrid g = single_grid(n_rays);
    hipLaunchKernelGGL((forbes_trace_kernel<T>), g.blocks, g.threads, 0, st, a);
  });
}
