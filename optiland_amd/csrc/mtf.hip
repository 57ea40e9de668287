// mtf.hip -- the geometric MTF of image-plane hits (ol_geometric_mtf).
//
// Reference: optiland/mtf/geometric.py:152-204 on the NumPy backend.  For every curve (the x or
// the y coordinates of one field's hits)
//
//   A, edges = np.histogram(x, bins = n_bins)          x_j = (edges[j + 1] + edges[j]) / 2
//   mtf_k    = scale_k |sum_j A_j exp(i 2 pi v_k x_j)| / sum_j A_j
//
// (W. J. Smith, Modern Optical Engineering, 3rd ed., section 11.9: the line spread function of
// the spot, transformed).  fp64 throughout; float32 coordinates are widened on load.  Three
// launches on the caller's stream, whatever the number of curves (blockIdx.y = curve):
//   1. range:     per block min / max / "a non-finite coordinate" of a slice of the curve, one
//                 partial per block; the bins of the curve are zeroed on the way;
//   2. histogram: every block folds the partials (the same min / max in every block), bins its
//                 slice into int32 LDS bins with NumPy's rule -- first guess
//                 (x - min) / (max - min) * n_bins, corrected by one against the two neighbouring
//                 edges of np.linspace(min, max, n_bins + 1) -- and adds its non-empty bins to
//                 the curve's global bins: INTEGER atomics, so arrival order does not matter;
//   3. transform: a block owns kFreq frequencies x kSlice interleaved slices of the bins; the
//                 slices' partial sums are added in slice order.
// The phase v_k x_j is carried in cycles and reduced exactly (t - rint(t), the product's low
// part kept); x_j is measured from the curve's minimum -- the modulus does not see the shift,
// and |x| of an off-axis field (tens of mm) times hundreds of cycles / mm stays out of the
// argument.  No float atomics: bit-identical from run to run, and a curve's result does not
// depend on the curves it shares a call with.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>

#include "../../include/optiland_hip.h"
#include "analysis_device.h"
#include "last_error.h"

// (namespace ol, not an anonymous one: tools/asm_stats.py and rocprofv3 name the kernels)
namespace ol {

constexpr int kMtfBlock = 256;                 // 4 waves
constexpr int kMtfMaxSlabs = 256;              // blocks per curve in passes 1 and 2 (<= kMtfBlock)
constexpr int64_t kMtfPerBlock = 256 * 16;     // points a block takes before another one is added
constexpr int kFreq = 16, kSlice = 16;         // pass 3: kFreq x kSlice = kMtfBlock
constexpr int kBinTile = 1024;                 // pass 3: bins staged in LDS at a time
static_assert(kFreq * kSlice == kMtfBlock && kBinTile % kSlice == 0, "pass 3 layout");
static_assert(kMtfMaxSlabs <= kMtfBlock, "pass 2 folds one partial per lane");

struct MtfCurves {
  const void* x[OL_MTF_MAX_CURVES];
  int64_t n[OL_MTF_MAX_CURVES];
};

struct MtfPartial {
  double lo, hi;
  int32_t bad, pad_;
};

// np.linspace(lo, hi, n_bins + 1)[j]: j * step + lo with the product rounded BEFORE the sum
// (numpy/_core/function_base.py: `y = y * step; y += start`; a step that underflowed to 0:
// `y /= div; y = y * delta`), the last edge exactly `hi`
struct MtfEdges {
  double lo, hi, step, delta;
  int n_bins;
  __device__ MtfEdges(double lo_, double hi_, int n) : lo(lo_), hi(hi_), n_bins(n) {
    delta = hi - lo;
    step = delta / (double)n;
  }
  __device__ __forceinline__ double operator()(int j) const {
#pragma clang fp contract(off)
    if (j >= n_bins) return hi;
    const double p = step != 0.0 ? (double)j * step : ((double)j / (double)n_bins) * delta;
    return p + lo;
  }
};

// the range np.histogram takes (numpy/lib/_histograms_impl.py `_get_outer_edges`): min and max,
// widened by a half when they coincide; (0, 1) for no point at all
__device__ __forceinline__ void mtf_outer_edges(double& lo, double& hi, int64_t n) {
  if (n == 0) {
    lo = 0.0;
    hi = 1.0;
  } else if (lo == hi) {
    lo -= 0.5;
    hi += 0.5;
  }
}

template <typename T>
__global__ __launch_bounds__(kMtfBlock) void mtf_range_kernel(MtfCurves curves, int n_bins,
                                                               MtfPartial* __restrict__ partial,
                                                               int32_t* __restrict__ counts) {
  const int c = blockIdx.y, tid = threadIdx.x;
  for (int j = blockIdx.x * kMtfBlock + tid; j < n_bins; j += gridDim.x * kMtfBlock)
    counts[(int64_t)c * n_bins + j] = 0;
  const T* __restrict__ x = (const T*)curves.x[c];
  const int64_t n = curves.n[c];
  double lo = std::numeric_limits<double>::infinity(), hi = -lo;
  int bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * kMtfBlock + tid; i < n;
       i += (int64_t)gridDim.x * kMtfBlock) {
    const double v = (double)x[i];
    bad |= !is_finite(v);
    lo = fmin(lo, v);
    hi = fmax(hi, v);
  }
  __shared__ double s_lo[kMtfBlock], s_hi[kMtfBlock];
  __shared__ int s_bad[kMtfBlock];
  s_lo[tid] = lo;
  s_hi[tid] = hi;
  s_bad[tid] = bad;
  __syncthreads();
  for (int w = kMtfBlock / 2; w > 0; w >>= 1) {
    if (tid < w) {
      s_lo[tid] = fmin(s_lo[tid], s_lo[tid + w]);
      s_hi[tid] = fmax(s_hi[tid], s_hi[tid + w]);
      s_bad[tid] |= s_bad[tid + w];
    }
    __syncthreads();
  }
  if (tid == 0) {
    MtfPartial p;
    p.lo = s_lo[0];
    p.hi = s_hi[0];
    p.bad = s_bad[0];
    p.pad_ = 0;
    partial[(int64_t)c * gridDim.x + blockIdx.x] = p;
  }
}

// dynamic LDS: n_bins int32 bins
template <typename T>
__global__ __launch_bounds__(kMtfBlock) void mtf_histogram_kernel(
    MtfCurves curves, int n_bins, const MtfPartial* __restrict__ partial,
    int32_t* __restrict__ counts, double* __restrict__ edges_minmax,
    int32_t* __restrict__ flags) {
  extern __shared__ __align__(16) int32_t s_bins[];
  __shared__ double s_lo[kMtfBlock], s_hi[kMtfBlock];
  __shared__ int s_bad[kMtfBlock];
  const int c = blockIdx.y, tid = threadIdx.x;
  const int slabs = gridDim.x;  // the same grid as pass 1: one partial per block
  {
    MtfPartial p;
    p.lo = std::numeric_limits<double>::infinity();
    p.hi = -p.lo;
    p.bad = 0;
    if (tid < slabs) p = partial[(int64_t)c * slabs + tid];
    s_lo[tid] = p.lo;
    s_hi[tid] = p.hi;
    s_bad[tid] = p.bad;
  }
  for (int j = tid; j < n_bins; j += kMtfBlock) s_bins[j] = 0;
  // (the fold of mtf_range_kernel, written out a second time: behind one inline function the
  // compiler lays this kernel's blocks out differently, and its code is no longer the measured one)
  __syncthreads();
  for (int w = kMtfBlock / 2; w > 0; w >>= 1) {
    if (tid < w) {
      s_lo[tid] = fmin(s_lo[tid], s_lo[tid + w]);
      s_hi[tid] = fmax(s_hi[tid], s_hi[tid + w]);
      s_bad[tid] |= s_bad[tid + w];
    }
    __syncthreads();
  }
  const int64_t n = curves.n[c];
  double lo = s_lo[0], hi = s_hi[0];
  const int bad = s_bad[0];
  if (!bad) mtf_outer_edges(lo, hi, n);
  if (blockIdx.x == 0 && tid == 0) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    edges_minmax[2 * c] = bad ? nan : lo;
    edges_minmax[2 * c + 1] = bad ? nan : hi;
    flags[c] = bad ? OL_MTF_NONFINITE : 0;
  }
  if (bad) return;  // (block-uniform) np.histogram raises for such a range: no bins
  const MtfEdges edge(lo, hi, n_bins);
  const T* __restrict__ x = (const T*)curves.x[c];
  const double denom = hi - lo;
  for (int64_t i = (int64_t)blockIdx.x * kMtfBlock + tid; i < n;
       i += (int64_t)gridDim.x * kMtfBlock) {
    const double v = (double)x[i];
    // numpy/lib/_histograms_impl.py:855-867
    const double f = ((v - lo) / denom) * (double)n_bins;
    int idx = (int)f;
    idx = std::min(std::max(idx, 0), n_bins - 1);  // (idx == n_bins: the closed last bin)
    if (v < edge(idx)) idx = std::max(idx - 1, 0);
    if (idx != n_bins - 1 && v >= edge(idx + 1)) ++idx;
    atomicAdd(&s_bins[idx], 1);
  }
  __syncthreads();
  for (int j = tid; j < n_bins; j += kMtfBlock) {
    const int32_t k = s_bins[j];
    if (k != 0) atomicAdd(&counts[(int64_t)c * n_bins + j], k);
  }
}

// grid = (ceil(num_points / kFreq), n_curves)
__global__ __launch_bounds__(kMtfBlock) void mtf_transform_kernel(
    int n_bins, int num_points, const double* __restrict__ freq,
    const double* __restrict__ scale, const int32_t* __restrict__ counts,
    const double* __restrict__ edges_minmax, const int32_t* __restrict__ flags,
    double* __restrict__ mtf) {
  __shared__ double s_a[kBinTile], s_d[kBinTile];
  __shared__ double s_re[kMtfBlock], s_im[kMtfBlock], s_n[kMtfBlock];
  const int c = blockIdx.y, tid = threadIdx.x;
  const int fl = tid % kFreq, sl = tid / kFreq;
  const int k = blockIdx.x * kFreq + fl;
  if (flags[c] != 0) {  // (block-uniform)
    if (sl == 0 && k < num_points)
      mtf[(int64_t)c * num_points + k] = std::numeric_limits<double>::quiet_NaN();
    return;
  }
  const double lo = edges_minmax[2 * c];
  const MtfEdges edge(lo, edges_minmax[2 * c + 1], n_bins);
  const double v = k < num_points ? freq[k] : 0.0;
  double re = 0.0, im = 0.0, total = 0.0;
  for (int base = 0; base < n_bins; base += kBinTile) {
    const int m = std::min(kBinTile, n_bins - base);
    __syncthreads();
    for (int i = tid; i < m; i += kMtfBlock) {
      const int j = base + i;
      s_a[i] = (double)counts[(int64_t)c * n_bins + j];
      s_d[i] = (edge(j + 1) + edge(j)) / 2 - lo;  // the bin centre, from the curve's minimum
    }
    __syncthreads();
    for (int i = sl; i < m; i += kSlice) {
      const double a = s_a[i], d = s_d[i];
      // the phase in cycles as t + t_lo
      const double t = v * d;
      const double t_lo = fma(v, d, -t);
      double sn, cs;
      sincospi(2.0 * phase_cycles(t, t_lo), &sn, &cs);
      re = fma(a, cs, re);
      im = fma(a, sn, im);
      total += a;  // (integers below 2^53: exact)
    }
  }
  s_re[tid] = re;
  s_im[tid] = im;
  s_n[tid] = total;
  __syncthreads();
  if (sl == 0 && k < num_points) {
    for (int s = 1; s < kSlice; ++s) {  // fixed order
      re += s_re[s * kFreq + fl];
      im += s_im[s * kFreq + fl];
      total += s_n[s * kFreq + fl];
    }
    const double m = hypot(re, im) / total;  // no point at all: 0 / 0, as in the reference
    mtf[(int64_t)c * num_points + k] = scale ? scale[k] * m : m;
  }
}

template <typename T>
static void mtf_launch(const MtfCurves& curves, int n_curves, unsigned slabs, int n_bins,
                       int num_points, const double* freq, const double* scale,
                       MtfPartial* partial, int32_t* counts, double* mtf, double* edges_minmax,
                       int32_t* flags, hipStream_t st) {
  const dim3 grid(slabs, (unsigned)n_curves);
  hipLaunchKernelGGL(mtf_range_kernel<T>, grid, dim3(kMtfBlock), 0, st, curves, n_bins, partial,
                     counts);
  hipLaunchKernelGGL(mtf_histogram_kernel<T>, grid, dim3(kMtfBlock),
                     (size_t)n_bins * sizeof(int32_t), st, curves, n_bins,
                     (const MtfPartial*)partial, counts, edges_minmax, flags);
  if (num_points > 0)
    hipLaunchKernelGGL(mtf_transform_kernel,
                       dim3((unsigned)((num_points + kFreq - 1) / kFreq), (unsigned)n_curves),
                       dim3(kMtfBlock), 0, st, n_bins, num_points, freq, scale,
                       (const int32_t*)counts, (const double*)edges_minmax,
                       (const int32_t*)flags, mtf);
}

}  // namespace ol

using namespace ol;

extern "C" int ol_geometric_mtf(ol_dtype dt, int32_t n_curves, const void* const* coords,
                                const int64_t* lengths, int32_t num_points, const double* freq,
                                const double* scale, int32_t n_bins, double* mtf_out,
                                int32_t* counts_out, double* edges_minmax_out,
                                int32_t* flags_out, void* stream) {
  if (dt != OL_F32 && dt != OL_F64)
    return failf(OL_EINVAL, "ol_geometric_mtf: dtype %d is neither OL_F32 nor OL_F64", (int)dt);
  if (n_curves < 0 || n_curves > OL_MTF_MAX_CURVES)
    return failf(OL_EINVAL, "ol_geometric_mtf: n_curves %d is outside 0..%d", (int)n_curves,
                 OL_MTF_MAX_CURVES);
  if (num_points < 0)
    return failf(OL_EINVAL, "ol_geometric_mtf: negative count (num_points %d)",
                 (int)num_points);
  if (n_bins < 1 || n_bins > OL_MTF_MAX_BINS)
    return failf(OL_EINVAL, "ol_geometric_mtf: n_bins %d is outside 1..%d", (int)n_bins,
                 OL_MTF_MAX_BINS);
  if (n_curves == 0) return OL_OK;
  if (!coords || !lengths) return failf(OL_EINVAL, "ol_geometric_mtf: NULL argument");
  if (!edges_minmax_out || !flags_out)
    return failf(OL_EINVAL, "ol_geometric_mtf: edges_minmax_out / flags_out is NULL");
  if (num_points > 0 && (!freq || !mtf_out))
    return failf(OL_EINVAL, "ol_geometric_mtf: freq / mtf_out is NULL");
  MtfCurves curves = {};
  int64_t longest = 0;
  for (int c = 0; c < n_curves; ++c) {
    if (lengths[c] < 0)
      return failf(OL_EINVAL, "ol_geometric_mtf: negative count (lengths[%d] = %lld)", c,
                   (long long)lengths[c]);
    if (lengths[c] > (int64_t)std::numeric_limits<int32_t>::max())
      return failf(OL_EINVAL, "ol_geometric_mtf: lengths[%d] = %lld does not fit the int32 bins",
                   c, (long long)lengths[c]);
    if (lengths[c] > 0 && !coords[c])
      return failf(OL_EINVAL, "ol_geometric_mtf: coords[%d] is NULL", c);
    curves.x[c] = coords[c];
    curves.n[c] = lengths[c];
    longest = std::max(longest, lengths[c]);
  }

  hipStream_t st = (hipStream_t)stream;
  const unsigned slabs = (unsigned)std::max<int64_t>(
      1, std::min<int64_t>((longest + kMtfPerBlock - 1) / kMtfPerBlock, kMtfMaxSlabs));
  const size_t partial_bytes = (size_t)n_curves * slabs * sizeof(MtfPartial);
  const size_t bytes =
      partial_bytes + (counts_out ? 0 : (size_t)n_curves * (size_t)n_bins * sizeof(int32_t));
  Workspace ws{"ol_geometric_mtf", st};
  if (int rc = ws.alloc(bytes)) return rc;
  MtfPartial* partial = (MtfPartial*)ws.ptr;
  int32_t* counts = counts_out ? counts_out : (int32_t*)((char*)ws.ptr + partial_bytes);
  if (dt == OL_F32)
    mtf_launch<float>(curves, n_curves, slabs, n_bins, num_points, freq, scale, partial, counts,
                      mtf_out, edges_minmax_out, flags_out, st);
  else
    mtf_launch<double>(curves, n_curves, slabs, n_bins, num_points, freq, scale, partial, counts,
                       mtf_out, edges_minmax_out, flags_out, st);
  return ws.finish();
}
