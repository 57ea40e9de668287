// grating.hip -- one diffraction grating on the device (ol_trace_grating).
//
// Reference: Surface.trace on PlaneGrating / StandardGratingGeometry with
// DiffractiveInteractionModel (surfaces/standard_surface.py:232-274,
// interactions/diffractive_model.py:28-61, rays/real_rays.py:207-522): gratingdiffract is about
// 150 lines of expanded polynomial, several hundred elementwise launches per surface on a device
// backend, each allocating an N-vector.  Here the surface is ONE launch between two fused runs of
// ol_trace: one ray per lane, the frame change, the intersection (no Newton loop), propagation,
// absorption, OPD and clip, the diffraction in its collected form (grating_device.h), a simple
// coating, the way back to the global frame and the stores of the ray state and of the recorded
// row.  Nothing is shared between lanes but the OR of the status word.  The fused kernels do not
// know these surfaces: their entry points refuse a range that holds one (entry_rules.h:
// rule_no_single_kinds).
//
// Shape of the launch: single_surface.h, shared with forbes.hip.
// 8 planes read, up to 16 written, some
// hundred fp operations per ray: at millions of rays the launch is bound by memory, at the
// thousands of rays of an Optic.trace by launch latency.  Table fields are wave-uniform scalar
// loads; no indexed memory access.  Compiled for gfx950 (tools/kernel_resources.py on the object):
//   grating_trace_kernel<float>    52 VGPRs, 88 SGPRs
//   grating_trace_kernel<double>   58 VGPRs, 74 SGPRs
// no scratch, no LDS, no spills.  Measured on the MI355X: profiles/grating.txt
// (tools/gpu_grating.py).
#include <hip/hip_runtime.h>

#include "../../include/optiland_hip.h"
#include "grating_device.h"
#include "grating_host.h"
#include "single_surface.h"

// (namespace ol, not an anonymous one: tools/asm_stats.py and rocprofv3 name the kernels)
namespace ol {

template <typename T>
struct GratingArgs : SingleArgs<T> {
  T wavelength;                 // micrometres
};

template <typename T>
__global__ __launch_bounds__(kSingleThreads) void grating_trace_kernel(GratingArgs<T> a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const Ray<T> r = single_load(a, i);
  const Ray<T> g = grating_step<T>(single_fetched(a), as_const(a.coeffs), r, a.wavelength);
  single_store(a, i, g);
  // evanescent order: a position without a direction (see OL_STATUS_NAN_DIRECTION)
  const bool report = a.status != nullptr && !(a.flags & OL_TRACE_MIDRANGE);   // (wave-uniform)
  if (report && g.L != g.L && g.x == g.x) atomicOr(a.status, kStatusNanDirection);
}

}  // namespace ol

using namespace ol;

extern "C" int ol_trace_grating(const ol_system* sys, ol_dtype dt, int64_t n_rays,
                                void* const rays[8], int32_t wavelength_index,
                                double wavelength_um, void* record_row, int64_t record_stride,
                                int32_t surface, uint32_t flags, uint32_t* status, void* stream) {
  if (int rc = grating_check(sys, dt, n_rays, rays, wavelength_index, wavelength_um, record_row,
                             record_stride, surface, flags))
    return rc;
  return single_entry(kSingleKinds[kSingleGrating].entry, sys, dt, n_rays, stream,
                      [&](auto t, const SystemView& v, hipStream_t st) {
    using T = decltype(t);
    const GratingArgs<T> a{single_args<T>(v, surface, wavelength_index, n_rays, rays, record_row,
                                          record_stride, flags, status),
                           (T)wavelength_um};
    const SingleGrid g = single_grid(n_rays);
    hipLaunchKernelGGL((grating_trace_kernel<T>), g.blocks, g.threads, 0, st, a);
  });
}
