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
// a range that holds one (entry_rules.h: rule_no_forbes).
//
// Shape of the launch.  8 planes read, up to 16 written, per ray some hundred fp operations per
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
#include "trace_launch.h"

// (namespace ol, not an anonymous one: tools/asm_stats.py and rocprofv3 name the kernels)
namespace ol {

constexpr int kForbesBlock = 256;

template <typename T>
struct ForbesArgs {
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
__global__ __launch_bounds__(kForbesBlock) void forbes_trace_kernel(ForbesArgs<T> a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;   // (the Newton loop's vote is among the lanes that stay)
  Ray<T> r;
  r.x = a.rays[0][i]; r.y = a.rays[1][i]; r.z = a.rays[2][i];
  r.L = a.rays[3][i]; r.M = a.rays[4][i]; r.N = a.rays[5][i];
  r.i = a.rays[6][i]; r.opd = a.rays[7][i];
  const SurfFetched<T> h{as_const(a.hot), as_const(a.cold), as_const(a.opt)};
  const Ray<T> g = forbes_step<T>(h, as_const(a.coeffs), r);
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
  // total internal reflection: a position without a direction (see OL_STATUS_NAN_DIRECTION)
  if (a.status != nullptr && !(a.flags & OL_TRACE_MIDRANGE) && g.L != g.L && g.x == g.x)
    atomicOr(a.status, kStatusNanDirection);
}

template <typename T>
void forbes_launch(const DevSurfHot<T>* hot, const DevSurfCold<T>* cold, const DevOptics<T>* opt,
                   const T* coeffs, int32_t surface, int32_t n_wl, int32_t wl, int64_t n,
                   void* const rays[8], void* row, int64_t stride, uint32_t flags,
                   uint32_t* status, hipStream_t st) {
  ForbesArgs<T> a{};
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
  const int block = n >= (int64_t)kForbesBlock * 256 ? kForbesBlock : 64;
  const unsigned blocks = (unsigned)((n + block - 1) / block);
  hipLaunchKernelGGL((forbes_trace_kernel<T>), dim3(blocks), dim3(block), 0, st, a);
}

}  // namespace ol

using namespace ol;

extern "C" int ol_trace_forbes(const ol_system* sys, ol_dtype dt, int64_t n_rays,
                               void* const rays[8], int32_t wavelength_index, void* record_row,
                               int64_t record_stride, int32_t surface, uint32_t flags,
                               uint32_t* status, void* stream) {
  if (int rc = forbes_check(sys, dt, n_rays, rays, wavelength_index, record_row, record_stride,
                            surface, flags))
    return rc;
  if (n_rays == 0) return OL_OK;
  const SystemView v = system_view(sys);
  if (int rc = rule_current_device("ol_trace_forbes", v)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (dt == OL_F32)
    forbes_launch<float>(v.surf32, v.cold32, v.optics32, v.coeffs32, surface, v.n_wl,
                         wavelength_index, n_rays, rays, record_row, record_stride, flags, status,
                         st);
  else
    forbes_launch<double>(v.surf, v.cold, v.optics, v.coeffs, surface, v.n_wl, wavelength_index,
                          n_rays, rays, record_row, record_stride, flags, status, st);
  Workspace ws{"ol_trace_forbes", st};
  return ws.finish();
}
