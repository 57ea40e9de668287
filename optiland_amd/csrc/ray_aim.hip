// ray_aim.hip -- iterative ray aiming on the device (ol_aim_rays).
//
// Reference: rays/ray_aiming/iterative.py:60-281 (`IterativeRayAimer.aim_rays`): up to max_iter
// Broyden steps, each a trace of the whole batch from the object to the stop surface by
// surface -- on a device backend ~100 array operations per surface and step, and a host
// synchronisation at every be.all / be.any.  The solve is independent per ray
// (ray_aim_device.h), so here it is ONE launch: one ray per lane, its launch state, trial
// state and Jacobian estimate in registers, nothing shared between lanes, the only atomic the
// OR of the status word.  fp64 only.
//
// Shape of the launch.  A call aims the rays of one Optic.trace -- tens to a few thousand --
// and each lane runs (max_iter + 1) x (stop - first + 1) surface steps in sequence: the launch
// is latency-bound and far too small to fill the device, so the workgroup is ONE wave (64):
// rays spread over as many compute units as there are waves, and the wave-uniform early exit
// (no lane active) is taken per 64 rays.  Two instantiations, as for the chief-ray kernel:
// conic-only ranges carry no Newton-Raphson code; everything else takes the generic one (a
// cold kernel: the single-family variants would buy registers nobody is short of at this
// occupancy).  Table rows are re-read phase by phase (SurfFetched), so nothing of a surface
// stays in SGPRs across the solve's loop.  Compiled for gfx950: 111 VGPRs (conic-only) and 166
// (generic), no scratch, no LDS.  Measured on the MI355X (profiles/ray_aim.txt,
// tools/gpu_ray_aim.py): 0.05-0.09 ms per call to the status read-back, at 37 rays and at 37 888.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/optiland_hip.h"
#include "last_error.h"
#include "ray_aim_device.h"
#include "ray_aim_host.h"
#include "raygen_device.h"
#include "system_view.h"
#include "trace_launch.h"

// (namespace ol, not an anonymous one: tools/asm_stats.py and rocprofv3 name the kernels)
namespace ol {

constexpr int kAimBlock = 64;

struct AimArgs {
  AimTable table;
  AimConsts consts;
  RaygenIn<double> in;        // px, py always; the rest when generating
  RaygenConsts<double> rgc;
  const double* guess[6];     // all NULL: generate the paraxial launch state
  double* out[6];
  int32_t* updates;
  uint32_t* status;
  int64_t n;
};

template <int NR>
__global__ __launch_bounds__(kAimBlock) void aim_rays_kernel(AimArgs a) {
  const int64_t lane = (int64_t)blockIdx.x * kAimBlock + threadIdx.x;
  const bool mine = lane < a.n;
  // a lane past the end solves the last ray again and stores nothing: the wave stays whole
  // (n >= 1: the host returns before launching an empty call)
  const int64_t i = mine ? lane : a.n - 1;
  uint32_t status = 0;
  double px = a.in.px[i], py = a.in.py[i], o[6];
  if (a.guess[0] != nullptr) {
#pragma unroll
    for (int k = 0; k < 6; ++k) o[k] = a.guess[k][i];
  } else {
    double tx = a.in.tx0, ty = a.in.ty0, vx = a.in.vx0, vy = a.in.vy0;
    if (a.in.hx != nullptr) {
      const double hx = a.in.hx[i], hy = a.in.hy[i];
      if ((a.in.flags & kRaygenCheckField) && (outside_unit(hx) || outside_unit(hy)))
        status |= kStatusFieldRange;
      raygen_field<double>(a.rgc, hx, hy, tx, ty);
    }
    if (a.in.vx != nullptr) {
      vx = a.in.vx[i];
      vy = a.in.vy[i];
    }
    raygen_pupil<double>(a.in.flags, vx, vy, px, py, status);
    raygen_one<double>(a.rgc, tx, ty, px, py, vx, vy, o);
  }
  int32_t updates = 0;
  status |= aim_one<NR>(a.table, a.consts, px, py, o, updates, status);
  if (mine) {
#pragma unroll
    for (int k = 0; k < 6; ++k) a.out[k][i] = o[k];
    if (a.updates != nullptr) a.updates[i] = updates;
    if (status) atomicOr(a.status, status);
  }
}

}  // namespace ol

using namespace ol;

extern "C" int ol_aim_rays(const ol_system* sys, int64_t n_rays, int32_t wavelength_index,
                           int32_t first_surface, int32_t stop_surface, const ol_aim_params* p,
                           const ol_raygen_inputs* in, const void* const guess[6],
                           void* const out[6], int32_t* updates, uint32_t* status,
                           void* stream) {
  if (int rc = aim_check(sys, n_rays, wavelength_index, first_surface, stop_surface, p, in, guess,
                         out, status))
    return rc;
  if (n_rays == 0) return OL_OK;
  if (n_rays > (int64_t)0x7fffffff * kAimBlock)
    return failf(OL_EINVAL, "ol_aim_rays: %lld rays are more than one launch takes",
                 (long long)n_rays);
  const SystemView v = system_view(sys);
  if (int rc = rule_current_device("ol_aim_rays", v)) return rc;
  AimArgs a{};
  a.table = AimTable{v.surf, v.cold, v.optics, v.coeffs, first_surface, stop_surface, v.n_wl,
                     wavelength_index};
  a.consts = AimConsts{p->stop_radius, p->jacobian, p->tol, p->max_iter, p->infinite != 0};
  a.in.px = static_cast<const double*>(in->px);
  a.in.py = static_cast<const double*>(in->py);
  a.in.flags = in->flags;
  if (guess) {
    for (int k = 0; k < 6; ++k) a.guess[k] = static_cast<const double*>(guess[k]);
    a.in.flags &= ~(kRaygenCheckField | kRaygenCheckPupil | kRaygenPrescalePupil);
  } else {
    const ol_raygen_params& g = p->raygen;
    const RaygenDev rg{g.object_infinite, g.field_kind, g.EPL,     g.EPD,    g.max_field, g.offset,
                       g.z_first,         g.tele_dz,    g.apod_a, g.apod_b, g.apod_kind};
    a.rgc = RaygenConsts<double>(rg);
    a.in.hx = static_cast<const double*>(in->hx);
    a.in.hy = static_cast<const double*>(in->hy);
    a.in.vx = static_cast<const double*>(in->vx);
    a.in.vy = static_cast<const double*>(in->vy);
    a.in.hx0 = in->hx0; a.in.hy0 = in->hy0;
    a.in.vx0 = in->vx0; a.in.vy0 = in->vy0;
    if (a.in.hx == nullptr) uniform_field_tangents<double>(rg, a.in);
  }
  for (int k = 0; k < 6; ++k) a.out[k] = static_cast<double*>(out[k]);
  a.updates = updates;
  a.status = status;
  a.n = n_rays;

  hipStream_t st = (hipStream_t)stream;
  const unsigned blocks = (unsigned)((n_rays + kAimBlock - 1) / kAimBlock);
  if (system_newton_family(sys, first_surface, stop_surface) == kNrNone)
    hipLaunchKernelGGL((aim_rays_kernel<kNrNone>), dim3(blocks), dim3(kAimBlock), 0, st, a);
  else
    hipLaunchKernelGGL((aim_rays_kernel<kNrGeneric>), dim3(blocks), dim3(kAimBlock), 0, st, a);
  Workspace ws{"ol_aim_rays", st};
  return ws.finish();
}
