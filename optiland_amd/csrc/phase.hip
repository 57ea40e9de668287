// phase.hip -- one phase-profile plane on the device (ol_trace_phase).
//
// Reference: Surface.trace on a Plane with PhaseInteractionModel
// (surfaces/standard_surface.py:232-274, interactions/phase_interaction_model.py:45-132, the
// profiles of optiland/phase/): the model for metalenses, diffractive and holographic elements.
// On a device backend the analytic profiles are some eighty elementwise launches per surface,
// each allocating an N-vector; the gridded ones a grid_sample and an autograd backward pass per
// surface per trace.  Here the surface is ONE launch between two fused runs of ol_trace: one ray
// per lane, the frame change, the plane hit, propagation, absorption, OPD and clip, the
// interaction in its collected form (phase_device.h), a simple coating, the efficiency, the way
// back to the global frame and the stores of the ray state and of the recorded row.  Nothing is
// shared between lanes but the OR of the status word.  The fused kernels do not know these
// surfaces: their entry points refuse a range that holds one (entry_rules.h:
// rule_no_single_kinds).
//
// Shape of the launch: single_surface.h, shared with forbes.hip.
// 8 planes read, up to 16 written:
// at millions of rays the launch is bound by memory, at the thousands of rays of an Optic.trace
// by launch latency.  Table fields are wave-uniform scalar loads, and so is the switch on the
// profile kind; the gridded profiles add the code base's only per-lane table access, four
// gathers from the node block (indices clamped before the load, values masked after it).
// Compiled for gfx950 (tools/kernel_resources.py on the object):
//   phase_trace_kernel<float>    46 VGPRs, 86 SGPRs
//   phase_trace_kernel<double>   62 VGPRs, 72 SGPRs
// no scratch, no LDS, no spills, 8 waves per SIMD.  Measured on the MI355X: profiles/phase.txt
// (tools/gpu_phase.py) -- 5.5-6.0 TB/s of the 24 planes at 1e7 rays; a 512 x 512 grid 3.3 / 4.3
// TB/s: there the gathers bind, not the planes.
#include <hip/hip_runtime.h>

#include "../../include/optiland_hip.h"
#include "phase_device.h"
#include "phase_host.h"
#include "single_surface.h"

// (namespace ol, not an anonymous one: tools/asm_stats.py and rocprofv3 name the kernels)
namespace ol {

template <typename T>
struct PhaseArgs : SingleArgs<T> {
  int32_t wl;                   // wavelength index: the scale of a height profile
  T q;                          // phase_q(wavelength_um), millimetres per radian
};

// (fp64: without the second bound the compiler takes 66 VGPRs, one wave per SIMD fewer; fp32 has
// all 8 at 46 VGPRs, and the same bound there only spills scalars)
template <typename T>
__global__ __launch_bounds__(kSingleThreads, sizeof(T) == 8 ? 8 : 1) void phase_trace_kernel(PhaseArgs<T> a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const Ray<T> r = single_load(a, i);
  const Ray<T> g = phase_step<T>(single_fetched(a), as_const(a.coeffs), a.coeffs, r, a.wl, a.q);
  single_store(a, i, g);
  // a position without a direction (see OL_STATUS_NAN_DIRECTION); an evanescent ray is not one:
  // it is clipped and keeps a finite direction, as in the reference
  const bool report = a.status != nullptr && !(a.flags & OL_TRACE_MIDRANGE);   // (wave-uniform)
  if (report && g.L != g.L && g.x == g.x) atomicOr(a.status, kStatusNanDirection);
}

}  // namespace ol

using namespace ol;

extern "C" int ol_trace_phase(const ol_system* sys, ol_dtype dt, int64_t n_rays,
                              void* const rays[8], int32_t wavelength_index, double wavelength_um,
                              void* record_row, int64_t record_stride, int32_t surface,
                              uint32_t flags, uint32_t* status, void* stream) {
  if (int rc = phase_check(sys, dt, n_rays, rays, wavelength_index, wavelength_um, record_row,
                           record_stride, surface, flags))
    return rc;
  return single_entry(kSingleKinds[kSinglePhase].entry, sys, dt, n_rays, stream,
                      [&](auto t, const SystemView& v, hipStream_t st) {
    using T = decltype(t);
    const PhaseArgs<T> a{single_args<T>(v, surface, wavelength_index, n_rays, rays, record_row,
                                        record_stride, flags, status),
                         wavelength_index, (T)phase_q(wavelength_um)};
    const SingleGrid g = single_grid(n_rays);
    hipLaunchKernelGGL((phase_trace_kernel<T>), g.blocks, g.threads, 0, st, a);
  });
}
