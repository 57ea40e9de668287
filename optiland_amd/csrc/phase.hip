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
// surfaces: their entry points refuse a range that holds one (entry_rules.h: rule_no_phase).
//
// Shape of the launch: that of grating_launch (grating.hip).  8 planes read, up to 16 written:
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
#include "trace_launch.h"

// (namespace ol, not an anonymous one: tools/asm_stats.py and rocprofv3 name the kernels)
namespace ol {

constexpr int kPhaseThreads = 256;

template <typename T>
struct PhaseArgs {
  const DevSurfHot<T>* hot;     // THE surface's rows
  const DevSurfCold<T>* cold;
  const DevOptics<T>* opt;      // its row at the traced wavelength
  const T* coeffs;              // the table's coefficient buffer
  T* rays[8];
  T* row;                       // NULL: nothing recorded
  int64_t stride, n;
  uint32_t* status;
  uint32_t flags;
  int32_t wl;                   // wavelength index: the scale of a height profile
  T q;                          // wavelength_um * 1e-3 / (2 pi), millimetres per radian
};

// (fp64: without the second bound the compiler takes 66 VGPRs, one wave per SIMD fewer; fp32 has
// all 8 at 46 VGPRs, and the same bound there only spills scalars)
template <typename T>
__global__ __launch_bounds__(kPhaseThreads, sizeof(T) == 8 ? 8 : 1) void phase_trace_kernel(PhaseArgs<T> a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  Ray<T> r;
  r.x = a.rays[0][i]; r.y = a.rays[1][i]; r.z = a.rays[2][i];
  r.L = a.rays[3][i]; r.M = a.rays[4][i]; r.N = a.rays[5][i];
  r.i = a.rays[6][i]; r.opd = a.rays[7][i];
  const SurfFetched<T> h{as_const(a.hot), as_const(a.cold), as_const(a.opt)};
  const Ray<T> g = phase_step<T>(h, as_const(a.coeffs), a.coeffs, r, a.wl, a.q);
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
  // a position without a direction (see OL_STATUS_NAN_DIRECTION); an evanescent ray is not one:
  // it is clipped and keeps a finite direction, as in the reference
  if (a.status != nullptr && !(a.flags & OL_TRACE_MIDRANGE) && g.L != g.L && g.x == g.x)
    atomicOr(a.status, kStatusNanDirection);
}

template <typename T>
void phase_launch(const DevSurfHot<T>* hot, const DevSurfCold<T>* cold, const DevOptics<T>* opt,
                  const T* coeffs, int32_t surface, int32_t n_wl, int32_t wl, double wavelength,
                  int64_t n, void* const rays[8], void* row, int64_t stride, uint32_t flags,
                  uint32_t* status, hipStream_t st) {
  PhaseArgs<T> a{};
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
  a.wl = wl;
  a.q = (T)phase_q(wavelength);
  // small calls: one wave per workgroup, so that the rays spread over the compute units
  const int block = n >= (int64_t)kPhaseThreads * 256 ? kPhaseThreads : 64;
  const unsigned blocks = (unsigned)((n + block - 1) / block);
  hipLaunchKernelGGL((phase_trace_kernel<T>), dim3(blocks), dim3(block), 0, st, a);
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
  if (n_rays == 0) return OL_OK;
  const SystemView v = system_view(sys);
  if (int rc = rule_current_device("ol_trace_phase", v)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (dt == OL_F32)
    phase_launch<float>(v.surf32, v.cold32, v.optics32, v.coeffs32, surface, v.n_wl,
                        wavelength_index, wavelength_um, n_rays, rays, record_row, record_stride,
                        flags, status, st);
  else
    phase_launch<double>(v.surf, v.cold, v.optics, v.coeffs, surface, v.n_wl, wavelength_index,
                         wavelength_um, n_rays, rays, record_row, record_stride, flags, status,
                         st);
  Workspace ws{"ol_trace_phase", st};
  return ws.finish();
}
