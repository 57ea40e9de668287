// huygens.hip -- the Huygens-Fresnel summation of the Huygens PSF (ol_huygens_psf).
//
// Reference: optiland/psf/huygens_fresnel_strategies.py:97-172 (NumbaSummation) and
// :184-274 (TorchSummation).  For image points P_m and pupil samples Q_j
//
//   field_m = sum_j a_j exp(i k (R_mj - opd_j)) / R_mj * 1/2 (1 + ((P_m - Q_j) . Q_j / Rp) / R_mj)
//   psf_m   = |field_m|^2,          k = 2 pi / lambda,  R_mj = |P_m - Q_j|
//
// fp64 throughout, and beyond it where the phase needs it: k R is ~1e6 rad, so P - Q, |P - Q|^2,
// R and 1 / lambda are each carried as hi + lo into the phase in cycles (see the loop).  Against
// the exact field the sum is good to (n_pupil + 32) 2^-52 sum_j |a_j q_mj / R_mj| per pixel
// (tests/test_gpu_huygens_exact.py).  Three launches on the caller's stream:
//   1. rays:    one 64-byte record per pupil sample {Q, Q / Rp, a exp(-i k opd)} -- the per-ray
//               phase is folded into a complex weight once, so a term evaluates ONE sin/cos;
//   2. partial: lanes own image pixels (kPix per lane, register-blocked), the pupil index is
//               wave-uniform, so every ray record is one scalar load shared by the wave; the
//               grid's y dimension splits the pupil into `n_split` chunks (one partial sum per
//               chunk and pixel) so that a small image still fills the machine;
//   3. finish:  per pixel, the chunks' partial sums added in chunk order, |.|^2.
// No atomics: the result depends only on (n_pupil, n_image), bit for bit from run to run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "../../include/optiland_hip.h"
#include "analysis_device.h"
#include "last_error.h"

// (namespace ol, not an anonymous one: tools/asm_stats.py and rocprofv3 name the kernels)
namespace ol {

constexpr int kBlock = 256;                 // 4 waves
constexpr int kPix = 2;                     // image pixels per lane
constexpr int kTile = kBlock * kPix;        // image pixels per workgroup
constexpr int64_t kTargetBlocks = 2048;     // partial-sum workgroups aimed for (256 CUs x 8)
constexpr int64_t kMinChunk = 32;           // fewest pupil samples per chunk
constexpr int64_t kMaxPartials = 1 << 26;   // n_split x n_image cap (1 GiB of partial sums)

struct alignas(16) HuygensRay {
  double u, v, w;     // pupil point Q
  double nx, ny, nz;  // Q / Rp: unit normal of the reference sphere
  double wr, wi;      // a exp(-i k opd)
};
static_assert(sizeof(HuygensRay) == 64, "one 64-byte record per pupil sample");

// a + b = s + e and a - b = s + e exactly (Knuth's TwoSum; no operation here may be contracted
// or reassociated, and none is: contraction only fuses a product into a sum)
__device__ __forceinline__ void two_sum(double a, double b, double& s, double& e) {
  s = a + b;
  const double bb = s - a;
  e = (a - (s - bb)) + (b - bb);
}
__device__ __forceinline__ void two_diff(double a, double b, double& s, double& e) {
  s = a - b;
  const double bb = s - a;
  e = (a - (s - bb)) - (b + bb);
}

__global__ __launch_bounds__(kBlock) void huygens_rays_kernel(
    int64_t n, const double* __restrict__ x, const double* __restrict__ y,
    const double* __restrict__ z, const double* __restrict__ amp,
    const double* __restrict__ amp_imag, const double* __restrict__ opd, double inv_wl,
    double Rp, HuygensRay* __restrict__ out) {
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < n;
       j += (int64_t)gridDim.x * kBlock) {
    double c, s;
    sincospi(2.0 * phase_cycles(-opd[j] * inv_wl), &s, &c);
    const double ar = amp[j], ai = amp_imag ? amp_imag[j] : 0.0;
    HuygensRay r;
    r.u = x[j];
    r.v = y[j];
    r.w = z[j];
    r.nx = r.u / Rp;
    r.ny = r.v / Rp;
    r.nz = r.w / Rp;
    r.wr = ar * c - ai * s;
    r.wi = ar * s + ai * c;
    out[j] = r;
  }
}

// grid = (ceil(n_image / kTile), n_split); partial[(chunk * n_image + m) * 2 + {0, 1}]
__global__ __launch_bounds__(kBlock) void huygens_partial_kernel(
    int64_t n_pupil, int64_t chunk, const HuygensRay* __restrict__ rays, int64_t n_image,
    const double* __restrict__ ix, const double* __restrict__ iy,
    const double* __restrict__ iz, double inv_wl, double inv_wl_lo,
    double* __restrict__ partial) {
  const int64_t m0 = (int64_t)blockIdx.x * kTile + threadIdx.x;
  double px[kPix], py[kPix], pz[kPix], re[kPix], im[kPix];
#pragma unroll
  for (int p = 0; p < kPix; ++p) {
    const int64_t m = std::min(m0 + (int64_t)p * kBlock, n_image - 1);  // tail lanes: a copy
    px[p] = ix[m];
    py[p] = iy[m];
    pz[p] = iz[m];
    re[p] = 0.0;
    im[p] = 0.0;
  }
  const int64_t j0 = (int64_t)blockIdx.y * chunk;
  const int64_t j1 = std::min(n_pupil, j0 + chunk);
  for (int64_t j = j0; j < j1; ++j) {
    const HuygensRay r = rays[j];  // wave-uniform address: scalar loads
#pragma unroll
    for (int p = 0; p < kPix; ++p) {
      // P - Q as hi + lo: the rounding of the difference alone (half an ulp of 54 mm is
      // 3.5e-15 mm, 4e-11 rad at 0.55 um) is as much as the rounding of R, see below
      double dx, dy, dz, dxl, dyl, dzl;
      two_diff(px[p], r.u, dx, dxl);
      two_diff(py[p], r.v, dy, dyl);
      two_diff(pz[p], r.w, dz, dzl);
      // |P - Q|^2 as r2 + r2l: the three squares and their two sums, each with its exact
      // rounding error, and the cross terms of the low parts
      const double sx = dx * dx, sy = dy * dy, sz = dz * dz;
      double r2, e1, e2;
      two_sum(sz, sy, r2, e1);
      two_sum(r2, sx, r2, e2);
      double r2l = fma(dx, dx, -sx) + fma(dy, dy, -sy) + fma(dz, dz, -sz) + (e1 + e2);
      r2l = fma(2.0 * dx, dxl, fma(2.0 * dy, dyl, fma(2.0 * dz, dzl, r2l)));
      // R and 1/R from one hardware reciprocal square root: a Goldschmidt step and a Newton
      // correction of R ...
      const double y0 = __builtin_amdgcn_rsq(r2);
      double g = r2 * y0, h = 0.5 * y0;
      const double e = fma(-g, h, 0.5);
      g = fma(g, e, g);
      h = fma(h, e, h);
      const double R = fma(fma(-g, g, r2), h, g);
      // ... then the part of R a double cannot hold: the residual |P - Q|^2 - R^2 (one fma: R^2
      // is within a few ulp of r2, so the difference rounds 2^-100 r2 down) over 2R.  It matters:
      // R / lambda ~ 1e5 cycles, half an ulp of R is 4e-11 rad.
      const double d = fma(-R, R, r2) + r2l;
      const double inv = h + h;
      // t = R / lambda in cycles as t + t_lo: R (R_hi + R_lo) times 1/lambda (hi + lo)
      const double t = R * inv_wl;
      const double t_lo = fma(R, inv_wl, -t) + fma(R, inv_wl_lo, (d * h) * inv_wl);
      double c, s;
      sincospi(2.0 * phase_cycles(t, t_lo), &s, &c);
      // obliquity 1/2 (1 + cos theta), cos theta = (P - Q) . Q / (Rp R), and the 1/R of the
      // spherical wave
      const double dot = fma(dx, r.nx, fma(dy, r.ny, dz * r.nz));
      const double q = 0.5 * inv * fma(dot, inv, 1.0);
      const double cq = c * q, sq = s * q;
      re[p] = fma(r.wr, cq, fma(-r.wi, sq, re[p]));
      im[p] = fma(r.wr, sq, fma(r.wi, cq, im[p]));
    }
  }
  double* out = partial + (int64_t)blockIdx.y * n_image * 2;
#pragma unroll
  for (int p = 0; p < kPix; ++p) {
    const int64_t m = m0 + (int64_t)p * kBlock;
    if (m < n_image) {
      out[2 * m] = re[p];
      out[2 * m + 1] = im[p];
    }
  }
}

__global__ __launch_bounds__(kBlock) void huygens_finish_kernel(
    int64_t n_image, int64_t n_split, const double* __restrict__ partial,
    double* __restrict__ psf, double* __restrict__ field) {
  for (int64_t m = (int64_t)blockIdx.x * kBlock + threadIdx.x; m < n_image;
       m += (int64_t)gridDim.x * kBlock) {
    double re = 0.0, im = 0.0;
    for (int64_t s = 0; s < n_split; ++s) {  // fixed order
      re += partial[(s * n_image + m) * 2];
      im += partial[(s * n_image + m) * 2 + 1];
    }
    psf[m] = re * re + im * im;
    if (field) {
      field[2 * m] = re;
      field[2 * m + 1] = im;
    }
  }
}

static unsigned grid_for(int64_t n) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + kBlock - 1) / kBlock, 8192));
}

}  // namespace ol

using namespace ol;

extern "C" int ol_huygens_psf(int64_t n_pupil, const double* const pupil[5],
                              const double* amp_imag, int64_t n_image,
                              const double* const image[3], double wavelength_mm, double Rp,
                              double* psf_out, double* field_out, void* stream) {
  if (!pupil || !image) return failf(OL_EINVAL, "ol_huygens_psf: NULL argument");
  if (n_pupil < 0 || n_image < 0)
    return failf(OL_EINVAL, "ol_huygens_psf: negative count (n_pupil %lld, n_image %lld)",
                 (long long)n_pupil, (long long)n_image);
  if (!(wavelength_mm > 0.0) || std::isinf(wavelength_mm))
    return failf(OL_EINVAL, "ol_huygens_psf: wavelength %g mm must be positive", wavelength_mm);
  if (Rp == 0.0 || std::isnan(Rp))
    return failf(OL_EINVAL, "ol_huygens_psf: reference sphere radius Rp %g must be non-zero", Rp);
  if (n_image == 0) return OL_OK;
  if (!psf_out) return failf(OL_EINVAL, "ol_huygens_psf: psf_out is NULL");
  for (int k = 0; k < 3; ++k)
    if (!image[k]) return failf(OL_EINVAL, "ol_huygens_psf: image[%d] is NULL", k);
  if (n_pupil > 0)
    for (int k = 0; k < 5; ++k)
      if (!pupil[k]) return failf(OL_EINVAL, "ol_huygens_psf: pupil[%d] is NULL", k);

  hipStream_t st = (hipStream_t)stream;
  const int64_t tiles = (n_image + kTile - 1) / kTile;
  int64_t n_split = 0, chunk = 0;
  if (n_pupil > 0) {
    n_split = std::max<int64_t>(1, (kTargetBlocks + tiles - 1) / tiles);
    n_split = std::min(n_split, (n_pupil + kMinChunk - 1) / kMinChunk);
    n_split = std::max<int64_t>(1, std::min(n_split, kMaxPartials / n_image));
    chunk = (n_pupil + n_split - 1) / n_split;
    n_split = (n_pupil + chunk - 1) / chunk;  // every chunk non-empty
  }
  const size_t ray_bytes = (size_t)n_pupil * sizeof(HuygensRay);
  const size_t bytes = ray_bytes + (size_t)n_split * (size_t)n_image * 2 * sizeof(double);
  Workspace ws{"ol_huygens_psf", st};
  if (int rc = ws.alloc(bytes)) return rc;  // (nothing to sum: no bytes, no allocation)
  HuygensRay* rays = (HuygensRay*)ws.ptr;
  double* partial = (double*)((char*)ws.ptr + ray_bytes);
  const double inv_wl = 1.0 / wavelength_mm;  // 1 / lambda = inv_wl + inv_wl_lo
  const double inv_wl_lo = -std::fma(wavelength_mm, inv_wl, -1.0) / wavelength_mm;
  if (n_pupil > 0) {
    hipLaunchKernelGGL(huygens_rays_kernel, dim3(grid_for(n_pupil)), dim3(kBlock), 0, st,
                       n_pupil, pupil[0], pupil[1], pupil[2], pupil[3], amp_imag, pupil[4],
                       inv_wl, Rp, rays);
    hipLaunchKernelGGL(huygens_partial_kernel, dim3((unsigned)tiles, (unsigned)n_split),
                       dim3(kBlock), 0, st, n_pupil, chunk, (const HuygensRay*)rays, n_image,
                       image[0], image[1], image[2], inv_wl, inv_wl_lo, partial);
  }
  hipLaunchKernelGGL(huygens_finish_kernel, dim3(grid_for(n_image)), dim3(kBlock), 0, st,
                     n_image, n_split, (const double*)partial, psf_out, field_out);
  return ws.finish();
}
