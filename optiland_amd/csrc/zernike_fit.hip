// zernike_fit.hip -- the Zernike decomposition of a sampled wavefront and the sampled MTF built
// on it (ol_zernike_fit, ol_zernike_eval, ol_sampled_mtf).
//
// Reference: optiland/zernike/base.py:42-102, 216-258 (the basis), zernike/fit.py:101-118 (the
// least-squares fit), mtf/sampled.py:108-207 (the overlap sum of the pupil with its shifted
// copy); Niu & Tian, Zernike polynomials and their applications, J. Opt. 24 (2022) 123001.
//
//   Z_j(x, y) = norm_j R_n^|m|(r) (cos m phi for m >= 0, sin |m| phi for m < 0),  phi = atan2(y, x)
//   R_n^|m|(r) = sum_k c_k r^(n - 2k),   c_k = (-1)^k (n-k)! / (k! ((n+|m|)/2-k)! ((n-|m|)/2-k)!)
//
// The HOST builds the term table (optiland_amd/zernike.py): per term its output column, (n, m),
// the number of radial coefficients, norm_j and the c_k as exact doubles, the terms GROUPED by
// ascending |m|.  A lane walks the table once per point: r^|m|, cos |m| phi and sin |m| phi
// advance by one multiplication / one rotation when |m| steps up, and the radial sum is a Horner
// chain in r^2.  The table is uniform across the wave: scalar loads.  At r = 0 the rotation
// starts from (cos, sin) = (1, 0) -- atan2(0, 0) = 0 -- and r^|m| = 0 for m != 0.
//
// Fit (five launches on the caller's stream, no floating-point atomics, every sum in a fixed
// order that depends on (n, K) only: bit-identical from run to run):
//   1. gram:   a block takes tiles of kZkTile points; 32 lanes evaluate the K basis values of a
//              point each into an LDS tile [A | z]; every lane then owns entries of the packed
//              upper triangle of [A | z]^T [A | z] and adds the tile's 32 products to the block's
//              partial.  Points with intensity <= 0 (zernike_opd.py:78-81) are rows of zeros.
//   2. merge:  the blocks' partials, added in block order.
//   3. solve:  one block: Jacobi scaling S = D G D with D = diag(G)^-1/2, Cholesky S = L L^T,
//              two triangular solves.  L and D are kept.
//   4. gram<residual>: A^T (z - A c), the residual formed per point in fp64.
//   5. refine: the same factor solves for the correction, which is added.
// Plain normal equations square the condition number: the first solution is off by about
// cond(S) 2^-53 max|c|, and the refinement step with the fp64 residual multiplies that by about
// cond(S) 2^-53 again, towards the floor cond_2(A) 2^-53 max|c| of a backward-stable
// least-squares solver.  What has to be small for that is cond(S), and the pivot test does not
// bound it: the smallest pivot of the factorisation is only an UPPER bound of the smallest
// eigenvalue of S.  Against exact coefficients (tests/test_gpu_zernike_conditioning.py, the
// figures in profiles/zernike_fit.txt) the one step keeps the perturbation bound
// cond_2(A) K 2^-52 max|c| with a margin of 460 x or more up to cond_2(A) = 3e5; fits whose
// smallest pivot is 1.5e-8 ... 7e-8, just above the test, have cond_2(A) = 1e6 ... 2.3e6 (cond(S)
// of a few 1e12) and keep it by 23 x down to 1.2 x (1.04e-8 against 1.27e-8 at a pivot of 1.5e-8).
// That is where the test has to stand for ONE step; a second one would leave 1e-11 there.
// The status word: fewer valid points than terms; a scaled pivot <= kZkPivotMin (rank
// deficient, or too ill-conditioned for one refinement step -- see above; such a problem
// belongs to an SVD); a non-finite input.  With a status the coefficients are NaN.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>

#include "../../include/optiland_hip.h"
#include "analysis_device.h"
#include "last_error.h"

// (namespace ol, not an anonymous one: tools/asm_stats.py and rocprofv3 name the kernels)
namespace ol {

constexpr int kZkBlock = 256;                    // 4 waves
constexpr int kZkTile = 32;                      // points of one LDS tile of the Gram pass
constexpr int kZkMaxBlocks = 256;                // blocks (= partials) of the Gram pass
constexpr int kZkStride = 1 + OL_ZK_MAX_RADIAL;  // doubles per term: norm, c_0 ... c_11
constexpr double kZkPivotMin = 1e-8;
constexpr int kSmtfMaxChunks = 256;              // point chunks (= partials) per frequency
static_assert(OL_ZK_MAX_TERMS * (OL_ZK_MAX_TERMS + 1) / 2 * 8 + 4 * OL_ZK_MAX_TERMS * 8 <= 65536,
              "the packed factor and its vectors fit the LDS of the solve kernels");
static_assert(kZkTile * (OL_ZK_MAX_TERMS + 1) * 8 <= 65536, "the Gram tile fits the LDS");
static_assert(kZkTile <= kZkBlock && OL_ZK_MAX_TERMS <= kZkBlock, "one lane per point / term");

struct ZkTable {
  const int32_t* __restrict__ ti;  // K x 4: column, n, m, number of radial coefficients
  const double* __restrict__ tf;   // K x kZkStride: norm, c_0 (highest power) ... c_s
  int K;
};

// emit(column, Z_column(x, y)) for every term of the table.  The table lives in device memory:
// a column, a coefficient count or an |m| outside its range is clamped, so that a damaged
// table gives wrong numbers but no access out of bounds and no endless loop.
template <typename Emit>
__device__ __forceinline__ void zk_basis(const ZkTable& tb, double x, double y, Emit&& emit) {
  const double r2 = x * x + y * y;
  const double r = sqrt(r2);
  const double c1 = r > 0.0 ? x / r : 1.0, s1 = r > 0.0 ? y / r : 0.0;
  double cm = 1.0, sm = 0.0, rp = 1.0;
  int mm = 0;
  for (int t = 0; t < tb.K; ++t) {
    const int col = std::min(std::max(tb.ti[4 * t], 0), tb.K - 1);
    const int m = tb.ti[4 * t + 2];
    const int am = std::min(std::abs(m), OL_ZK_MAX_M);
    const int nc = std::min(std::max(tb.ti[4 * t + 3], 1), OL_ZK_MAX_RADIAL);
    while (mm < am) {  // (uniform) cos / sin of (mm + 1) phi by one rotation, r^(mm + 1)
      const double c = cm * c1 - sm * s1;
      sm = sm * c1 + cm * s1;
      cm = c;
      rp *= r;
      ++mm;
    }
    const double* __restrict__ f = tb.tf + (int64_t)t * kZkStride;
    double v = f[1];
    for (int k = 1; k < nc; ++k) v = fma(v, r2, f[1 + k]);
    emit(col, f[0] * (v * rp) * (m >= 0 ? cm : sm));
  }
}

__device__ __forceinline__ double zk_sum(const ZkTable& tb, const double* __restrict__ coeffs,
                                         double x, double y) {
  double w = 0.0;
  zk_basis(tb, x, y, [&](int col, double v) { w = fma(coeffs[col], v, w); });
  return w;
}

// packed triangle: entry (row b, column a <= b) at b (b + 1) / 2 + a
__device__ __forceinline__ int zk_packed(int b, int a) { return b * (b + 1) / 2 + a; }

// dynamic LDS: kZkTile x (K + 1) doubles.  kResidual = false: partial[block][e] over the whole
// packed triangle of the K + 1 columns [A | z]; true: partial[block][a] = sum A_a (z - A c).
// meta[block] = (valid points, a non-finite input) -- written by the first mode only.
template <bool kResidual>
__global__ __launch_bounds__(kZkBlock) void zk_gram_kernel(
    ZkTable tb, int64_t n, const double* __restrict__ x, const double* __restrict__ y,
    const double* __restrict__ z, const double* __restrict__ intensity,
    const double* __restrict__ coeffs, const int32_t* __restrict__ status,
    double* __restrict__ partial, int64_t* __restrict__ meta) {
  extern __shared__ __align__(16) double s_tile[];
  const int tid = threadIdx.x, K = tb.K, M = K + 1;
  const int entries = kResidual ? K : zk_packed(M, 0);
  double* __restrict__ mine = partial + (int64_t)blockIdx.x * entries;
  for (int e = tid; e < entries; e += kZkBlock) mine[e] = 0.0;
  if (kResidual && status[0] != 0) return;  // (uniform) no coefficients to refine
  const int64_t tiles = (n + kZkTile - 1) / kZkTile;
  int64_t count = 0;
  int bad = 0;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    __syncthreads();
    if (tid < kZkTile) {
      const int64_t i = tile * kZkTile + tid;
      double* __restrict__ row = s_tile + tid * M;
      bool valid = i < n;
      if (valid && intensity) valid = intensity[i] > 0.0;
      if (valid) {
        const double px = x[i], py = y[i], pz = z[i];
        bad |= !(is_finite(px) && is_finite(py) && is_finite(pz));
        ++count;
        if (kResidual) {
          double w = 0.0;
          zk_basis(tb, px, py, [&](int col, double v) {
            row[col] = v;
            w = fma(coeffs[col], v, w);
          });
          row[K] = pz - w;
        } else {
          zk_basis(tb, px, py, [&](int col, double v) { row[col] = v; });
          row[K] = pz;
        }
      } else {
        for (int c = 0; c < M; ++c) row[c] = 0.0;
      }
    }
    __syncthreads();
    for (int e = tid; e < entries; e += kZkBlock) {
      int a, b;
      if (kResidual) {
        a = e;
        b = K;
      } else {
        b = (int)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
        while (zk_packed(b + 1, 0) <= e) ++b;
        while (zk_packed(b, 0) > e) --b;
        a = e - zk_packed(b, 0);
      }
      double s = 0.0;
#pragma unroll 8
      for (int p = 0; p < kZkTile; ++p) s = fma(s_tile[p * M + a], s_tile[p * M + b], s);
      mine[e] += s;
    }
  }
  if (!kResidual) {
    __shared__ int64_t s_count[kZkTile];
    __shared__ int s_bad[kZkTile];
    __syncthreads();
    if (tid < kZkTile) {
      s_count[tid] = count;
      s_bad[tid] = bad;
    }
    __syncthreads();
    if (tid == 0) {
      for (int p = 1; p < kZkTile; ++p) {
        count += s_count[p];
        bad |= s_bad[p];
      }
      meta[2 * blockIdx.x] = count;
      meta[2 * blockIdx.x + 1] = bad;
    }
  }
}

// gram[e] = sum over the blocks, in block order; meta_out = (valid points, non-finite)
__global__ __launch_bounds__(kZkBlock) void zk_merge_kernel(
    int entries, int blocks, const double* __restrict__ partial, const int64_t* __restrict__ meta,
    double* __restrict__ gram, int64_t* __restrict__ meta_out) {
  const int e = blockIdx.x * kZkBlock + threadIdx.x;
  if (e < entries) {
    double s = 0.0;
    for (int g = 0; g < blocks; ++g) s += partial[(int64_t)g * entries + e];
    gram[e] = s;
  }
  if (e == 0) {
    int64_t count = 0, bad = 0;
    for (int g = 0; g < blocks; ++g) {
      count += meta[2 * g];
      bad |= meta[2 * g + 1];
    }
    meta_out[0] = count;
    meta_out[1] = bad;
  }
}

// v <- (L L^T)^-1 v with the packed factor in LDS; every lane of the block calls it
__device__ void zk_cholesky_solve(const double* s_l, double* s_v, int K, int tid) {
  for (int j = 0; j < K; ++j) {  // L w = v
    if (tid == 0) s_v[j] /= s_l[zk_packed(j, j)];
    __syncthreads();
    const double vj = s_v[j];
    for (int i = j + 1 + tid; i < K; i += kZkBlock) s_v[i] = fma(-s_l[zk_packed(i, j)], vj, s_v[i]);
    __syncthreads();
  }
  for (int j = K - 1; j >= 0; --j) {  // L^T u = w
    if (tid == 0) s_v[j] /= s_l[zk_packed(j, j)];
    __syncthreads();
    const double vj = s_v[j];
    for (int i = tid; i < j; i += kZkBlock) s_v[i] = fma(-s_l[zk_packed(j, i)], vj, s_v[i]);
    __syncthreads();
  }
}

// one block.  gram: the packed triangle of [A | z]^T [A | z]; factor_out: the packed L and,
// behind it, the K scale factors.
__global__ __launch_bounds__(kZkBlock) void zk_solve_kernel(
    int K, const double* __restrict__ gram, const int64_t* __restrict__ meta,
    double* __restrict__ factor_out, double* __restrict__ coeffs, int32_t* __restrict__ status) {
  __shared__ double s_l[OL_ZK_MAX_TERMS * (OL_ZK_MAX_TERMS + 1) / 2];
  __shared__ double s_d[OL_ZK_MAX_TERMS], s_v[OL_ZK_MAX_TERMS];
  __shared__ int s_status;
  const int tid = threadIdx.x;
  const int tri = zk_packed(K, 0);
  if (tid == 0) {
    int st = 0;
    if (meta[1] != 0) st |= OL_ZK_NONFINITE;
    if (meta[0] < (int64_t)K) st |= OL_ZK_TOO_FEW;
    s_status = st;
  }
  __syncthreads();
  if (s_status == 0) {
    if (tid < K) {
      const double g = gram[zk_packed(tid, tid)];
      s_d[tid] = g > 0.0 ? 1.0 / sqrt(g) : 0.0;
    }
    __syncthreads();
    if (tid < K) {
      if (s_d[tid] == 0.0) s_status = OL_ZK_RANK_DEFICIENT;  // a column of zeros (benign race)
      s_v[tid] = gram[tri + tid] * s_d[tid];
    }
    for (int b = 0; b < K; ++b)
      for (int a = tid; a <= b; a += kZkBlock)
        s_l[zk_packed(b, a)] = gram[zk_packed(b, a)] * s_d[a] * s_d[b];
    __syncthreads();
  }
  // right-looking Cholesky of the scaled matrix, a 16 x 16 lane grid over the trailing block
  const int ty = tid / 16, tx = tid % 16;
  for (int j = 0; j < K && s_status == 0; ++j) {
    const double pivot = s_l[zk_packed(j, j)];
    __syncthreads();  // (everybody has read the pivot and the status)
    if (!(pivot > kZkPivotMin)) {
      if (tid == 0) s_status = OL_ZK_RANK_DEFICIENT;
      __syncthreads();
      break;
    }
    const double ljj = sqrt(pivot);
    for (int i = j + 1 + tid; i < K; i += kZkBlock) s_l[zk_packed(i, j)] /= ljj;
    if (tid == 0) s_l[zk_packed(j, j)] = ljj;
    __syncthreads();
    for (int i = j + 1 + ty; i < K; i += 16) {
      const double lij = s_l[zk_packed(i, j)];
      for (int k = j + 1 + tx; k <= i; k += 16)
        s_l[zk_packed(i, k)] = fma(-lij, s_l[zk_packed(k, j)], s_l[zk_packed(i, k)]);
    }
    __syncthreads();
  }
  __syncthreads();
  const int st = s_status;
  if (st == 0) {
    zk_cholesky_solve(s_l, s_v, K, tid);
    for (int e = tid; e < tri; e += kZkBlock) factor_out[e] = s_l[e];
    if (tid < K) {
      factor_out[tri + tid] = s_d[tid];
      coeffs[tid] = s_v[tid] * s_d[tid];
    }
  } else if (tid < K) {
    coeffs[tid] = std::numeric_limits<double>::quiet_NaN();
  }
  if (tid == 0) status[0] = st;
}

// one block: coeffs += D (L L^T)^-1 D sum_g partial[g] (the partials added in block order)
__global__ __launch_bounds__(kZkBlock) void zk_refine_kernel(
    int K, int blocks, const double* __restrict__ partial, const double* __restrict__ factor,
    double* __restrict__ coeffs, const int32_t* __restrict__ status) {
  __shared__ double s_l[OL_ZK_MAX_TERMS * (OL_ZK_MAX_TERMS + 1) / 2];
  __shared__ double s_v[OL_ZK_MAX_TERMS];
  if (status[0] != 0) return;  // (uniform)
  const int tid = threadIdx.x;
  const int tri = zk_packed(K, 0);
  for (int e = tid; e < tri; e += kZkBlock) s_l[e] = factor[e];
  double d = 0.0;
  if (tid < K) {
    double s = 0.0;
    for (int g = 0; g < blocks; ++g) s += partial[(int64_t)g * K + tid];
    d = factor[tri + tid];
    s_v[tid] = s * d;
  }
  __syncthreads();
  zk_cholesky_solve(s_l, s_v, K, tid);
  if (tid < K) coeffs[tid] += s_v[tid] * d;
}

__global__ __launch_bounds__(kZkBlock) void zk_eval_kernel(ZkTable tb,
                                                           const double* __restrict__ coeffs,
                                                           int64_t n, const double* __restrict__ x,
                                                           const double* __restrict__ y,
                                                           double* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * kZkBlock + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kZkBlock)
    out[i] = zk_sum(tb, coeffs, x[i], y[i]);
}

// the reference's mask `sqrt(xs**2 + ys**2) > 1.0`, every operation rounded as NumPy rounds it:
// with the sum of squares contracted into an fma, points within two ulp of the rim land on the
// other side, and each of them moves the MTF by 1 / n
__device__ __forceinline__ bool smtf_outside(double xs, double ys) {
#pragma clang fp contract(off)
  const double xx = xs * xs, yy = ys * ys;
  return sqrt(xx + yy) > 1.0;
}

// grid = (point chunks, frequencies); partial[f][chunk] = (re, im, sum of the intensity)
__global__ __launch_bounds__(kZkBlock) void smtf_kernel(
    ZkTable tb, const double* __restrict__ coeffs, int64_t n, const double* __restrict__ x,
    const double* __restrict__ y, const double* __restrict__ opd, const double* __restrict__ p1,
    const double* __restrict__ intensity, const double* __restrict__ shifts,
    double* __restrict__ partial) {
  __shared__ double s_re[kZkBlock], s_im[kZkBlock], s_in[kZkBlock];
  const int tid = threadIdx.x, f = blockIdx.y;
  const double dx = shifts[2 * f], dy = shifts[2 * f + 1];
  double re = 0.0, im = 0.0, total = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kZkBlock + tid; i < n;
       i += (int64_t)gridDim.x * kZkBlock) {
    const double w = intensity[i];
    total += w;
    const double xs = x[i] - dx, ys = y[i] - dy;
    if (smtf_outside(xs, ys)) continue;  // sampled.py:190-193 (a NaN stays in)
    const double amp = sqrt(w);
    // the phase in cycles
    const double t = (p1 ? 0.0 : opd[i]) - zk_sum(tb, coeffs, xs, ys);
    double sn, cs;
    sincospi(2.0 * phase_cycles(t), &sn, &cs);
    if (p1) {  // (uniform) a pupil function the caller supplies: P1 sqrt(I) exp(-2 pi i W)
      const double pr = p1[2 * i], pj = p1[2 * i + 1];
      re += amp * (pr * cs - pj * sn);
      im += amp * (pr * sn + pj * cs);
    } else {
      re = fma(amp * amp, cs, re);
      im = fma(amp * amp, sn, im);
    }
  }
  s_re[tid] = re;
  s_im[tid] = im;
  s_in[tid] = total;
  __syncthreads();
  for (int w = kZkBlock / 2; w > 0; w >>= 1) {
    if (tid < w) {
      s_re[tid] += s_re[tid + w];
      s_im[tid] += s_im[tid + w];
      s_in[tid] += s_in[tid + w];
    }
    __syncthreads();
  }
  if (tid == 0) {
    double* __restrict__ p = partial + 3 * ((int64_t)f * gridDim.x + blockIdx.x);
    p[0] = s_re[0];
    p[1] = s_im[0];
    p[2] = s_in[0];
  }
}

__global__ __launch_bounds__(kZkBlock) void smtf_finish_kernel(int n_freq, int chunks,
                                                               const double* __restrict__ partial,
                                                               double* __restrict__ mtf,
                                                               double* __restrict__ otf) {
  const int f = blockIdx.x * kZkBlock + threadIdx.x;
  if (f >= n_freq) return;
  double re = 0.0, im = 0.0, total = 0.0;
  for (int c = 0; c < chunks; ++c) {  // fixed order
    const double* __restrict__ p = partial + 3 * ((int64_t)f * chunks + c);
    re += p[0];
    im += p[1];
    total += p[2];
  }
  if (total == 0.0) {  // sampled.py:199-200
    re = im = 0.0;
  } else {
    re /= total;
    im /= total;
  }
  mtf[f] = hypot(re, im);
  if (otf) {
    otf[2 * f] = re;
    otf[2 * f + 1] = im;
  }
}

static int zk_check_table(const char* who, int32_t num_terms, const int32_t* term_i,
                          const double* term_f) {
  if (num_terms < 1 || num_terms > OL_ZK_MAX_TERMS)
    return failf(OL_EINVAL, "%s: num_terms %d is outside 1..%d (OL_ZK_MAX_TERMS)", who,
                 (int)num_terms, OL_ZK_MAX_TERMS);
  if (!term_i || !term_f) return failf(OL_EINVAL, "%s: the term table is NULL", who);
  return OL_OK;
}

static int zk_check_count(const char* who, int64_t n) {
  if (n < 0) return failf(OL_EINVAL, "%s: negative count (n = %lld)", who, (long long)n);
  if (n > (int64_t)std::numeric_limits<int32_t>::max())
    return failf(OL_EINVAL, "%s: n = %lld is above INT32_MAX", who, (long long)n);
  return OL_OK;
}

}  // namespace ol

using namespace ol;

extern "C" int ol_zernike_fit(int32_t num_terms, const int32_t* term_i, const double* term_f,
                              int64_t n, const double* x, const double* y, const double* z,
                              const double* intensity, double* coeffs_out, int32_t* status_out,
                              void* stream) {
  if (int rc = zk_check_table("ol_zernike_fit", num_terms, term_i, term_f)) return rc;
  if (int rc = zk_check_count("ol_zernike_fit", n)) return rc;
  if (!coeffs_out || !status_out)
    return failf(OL_EINVAL, "ol_zernike_fit: coeffs_out / status_out is NULL");
  if (n > 0 && (!x || !y || !z)) return failf(OL_EINVAL, "ol_zernike_fit: x / y / z is NULL");

  hipStream_t st = (hipStream_t)stream;
  const int K = num_terms, M = K + 1;
  const int entries = M * (M + 1) / 2, tri = K * (K + 1) / 2;
  const int64_t tiles = (n + kZkTile - 1) / kZkTile;
  const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(tiles, kZkMaxBlocks));
  // workspace (doubles): partials | merged triangle | factor and scale | block and merged meta
  const size_t n_partial = (size_t)blocks * entries;
  const size_t doubles = n_partial + entries + tri + K + 2 * (size_t)blocks + 2;
  Workspace ws{"ol_zernike_fit", st};
  if (int rc = ws.alloc(doubles * sizeof(double))) return rc;
  double* partial = (double*)ws.ptr;
  double* gram = partial + n_partial;
  double* factor = gram + entries;
  int64_t* meta = (int64_t*)(factor + tri + K);
  int64_t* meta_all = meta + 2 * (size_t)blocks;
  const ZkTable tb = {term_i, term_f, K};
  const size_t lds = (size_t)kZkTile * M * sizeof(double);
  hipLaunchKernelGGL(zk_gram_kernel<false>, dim3(blocks), dim3(kZkBlock), lds, st, tb, n, x, y, z,
                     intensity, (const double*)nullptr, (const int32_t*)nullptr, partial, meta);
  hipLaunchKernelGGL(zk_merge_kernel, dim3((entries + kZkBlock - 1) / kZkBlock), dim3(kZkBlock), 0,
                     st, entries, blocks, (const double*)partial, (const int64_t*)meta, gram,
                     meta_all);
  hipLaunchKernelGGL(zk_solve_kernel, dim3(1), dim3(kZkBlock), 0, st, K, (const double*)gram,
                     (const int64_t*)meta_all, factor, coeffs_out, status_out);
  hipLaunchKernelGGL(zk_gram_kernel<true>, dim3(blocks), dim3(kZkBlock), lds, st, tb, n, x, y, z,
                     intensity, (const double*)coeffs_out, (const int32_t*)status_out, partial,
                     (int64_t*)nullptr);
  hipLaunchKernelGGL(zk_refine_kernel, dim3(1), dim3(kZkBlock), 0, st, K, blocks,
                     (const double*)partial, (const double*)factor, coeffs_out,
                     (const int32_t*)status_out);
  return ws.finish();
}

extern "C" int ol_zernike_eval(int32_t num_terms, const int32_t* term_i, const double* term_f,
                               const double* coeffs, int64_t n, const double* x, const double* y,
                               double* out, void* stream) {
  if (int rc = zk_check_table("ol_zernike_eval", num_terms, term_i, term_f)) return rc;
  if (int rc = zk_check_count("ol_zernike_eval", n)) return rc;
  if (!coeffs) return failf(OL_EINVAL, "ol_zernike_eval: coeffs is NULL");
  if (n == 0) return OL_OK;
  if (!x || !y || !out) return failf(OL_EINVAL, "ol_zernike_eval: x / y / out is NULL");
  const ZkTable tb = {term_i, term_f, num_terms};
  const unsigned blocks = (unsigned)std::min<int64_t>((n + kZkBlock - 1) / kZkBlock, 4096);
  hipLaunchKernelGGL(zk_eval_kernel, dim3(blocks), dim3(kZkBlock), 0, (hipStream_t)stream, tb,
                     coeffs, n, x, y, out);
  return Workspace{"ol_zernike_eval", (hipStream_t)stream}.finish();  // (no workspace)
}

extern "C" int ol_sampled_mtf(int32_t num_terms, const int32_t* term_i, const double* term_f,
                              const double* coeffs, int64_t n, const double* x, const double* y,
                              const double* opd_waves, const double* p1, const double* intensity,
                              int32_t n_freq, const double* shifts, double* mtf_out,
                              double* otf_out, void* stream) {
  if (int rc = zk_check_table("ol_sampled_mtf", num_terms, term_i, term_f)) return rc;
  if (int rc = zk_check_count("ol_sampled_mtf", n)) return rc;
  if (n_freq < 0 || n_freq > OL_SMTF_MAX_FREQ)
    return failf(OL_EINVAL, "ol_sampled_mtf: n_freq %d is outside 0..%d", (int)n_freq,
                 OL_SMTF_MAX_FREQ);
  if (!coeffs) return failf(OL_EINVAL, "ol_sampled_mtf: coeffs is NULL");
  if (n_freq == 0) return OL_OK;
  if (!shifts || !mtf_out) return failf(OL_EINVAL, "ol_sampled_mtf: shifts / mtf_out is NULL");
  if (n > 0 && (!x || !y || !intensity))
    return failf(OL_EINVAL, "ol_sampled_mtf: x / y / intensity is NULL");
  if (n > 0 && !opd_waves && !p1)
    return failf(OL_EINVAL, "ol_sampled_mtf: neither opd_waves nor p1 is given");

  hipStream_t st = (hipStream_t)stream;
  const int chunks = (int)std::max<int64_t>(
      1, std::min<int64_t>((n + kZkBlock - 1) / kZkBlock, kSmtfMaxChunks));
  const size_t bytes = (size_t)n_freq * chunks * 3 * sizeof(double);
  Workspace ws{"ol_sampled_mtf", st};
  if (int rc = ws.alloc(bytes)) return rc;
  const ZkTable tb = {term_i, term_f, num_terms};
  hipLaunchKernelGGL(smtf_kernel, dim3((unsigned)chunks, (unsigned)n_freq), dim3(kZkBlock), 0, st,
                     tb, coeffs, n, x, y, opd_waves, p1, intensity, shifts, (double*)ws.ptr);
  hipLaunchKernelGGL(smtf_finish_kernel, dim3((n_freq + kZkBlock - 1) / kZkBlock), dim3(kZkBlock),
                     0, st, (int)n_freq, chunks, (const double*)ws.ptr, mtf_out, otf_out);
  return ws.finish();
}
