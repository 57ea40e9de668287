// mmdft.hip -- the matrix-multiply DFT of the MMDFT PSF (ol_mmdft_psf).
//
// Reference: optiland/psf/mmdft.py:157-201 (_compute_psf, _get_normalization) and :223-283
// (_compute_kernels).  For a pupil g of N x N complex samples, an image of M x M pixels and a
// (real) pad size
//
//   cp_j = j - N/2,  ci_v = v - M/2  (integer division),    W[v][j] = exp(-2 pi i ci_v cp_j / pad)
//   T[y][u] = sum_x g[y][x] W[u][x]                         (rows:    T = g W^T, N x M)
//   G[v][u] = sum_y W[v][y] T[y][u]                         (columns: G = W T,   M x M)
//   psf[v][u] = |G[v][u]|^2 100 / c^2,                      c = #{cells with |g| > 0}
//
// The reference's L is W and its R is W^T, so ONE table serves both products.  Launches per
// slice of up to kSlice pupils (the pupil index is the grid's z dimension; the pad sizes of a
// slice travel as a kernel argument), all on the caller's stream:
//   1. table:   W, M x N complex128.  k = ci cp is an exact integer; the phase in cycles is
//               t = k / pad carried as t + t_lo (t_lo = fma(-t, pad, k) / pad, the remainder of
//               the division, which fp64 holds exactly), reduced exactly and handed to sincospi:
//               an entry is good to 3 ulp of 1 whatever |k / pad| is;
//      count:   c, an integer sum (integer atomics: the order cannot show);
//   2. rows:    a tiled complex fp64 product, 64 x 64 outputs per workgroup, 4 x 4 per lane,
//               LDS tiles of 16 along the reduction, the next tile's global loads in flight
//               while the current one is multiplied;
//   3. columns: the same kernel with T read row-wise and the epilogue |G|^2 100 / c^2 (and G
//               itself when the caller wants it).
// The reduction runs in index order in one accumulator per output: a result depends on (N, M)
// and the inputs only, bit for bit.  Plain v_fma_f64: the 4 x 4 register block takes as many
// LDS cycles as FMA cycles per step (8 ds_read_b128 against 64 fp64 FMAs per wave); measured,
// the columns product runs at 44 TFLOP/s at (N 181, M 2048) (profiles/mmdft.txt).  An fp64 MFMA
// variant was not built.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "../../include/optiland_hip.h"
#include "analysis_device.h"
#include "last_error.h"

// (namespace ol, not an anonymous one: tools/asm_stats.py and rocprofv3 name the kernels)
namespace ol {

constexpr int kMmBlock = 256;   // 4 waves: 16 x 16 lanes
constexpr int kMmTile = 64;     // outputs per workgroup and side
constexpr int kMmReg = 4;       // outputs per lane and side (rows ty + 16 i, columns tx + 16 j)
constexpr int kMmDepth = 16;    // reduction indices per LDS tile
constexpr int kMmRow = kMmTile + 1;  // padded LDS row: a store's depth indices spread over the banks
constexpr int kSlice = 32;      // pupils per launch (their pad sizes are a kernel argument)
static_assert(kMmTile == 16 * kMmReg && kMmBlock * 4 == kMmTile * kMmDepth, "tile geometry");

struct MmdftPads {
  double v[kSlice];
};

// grid = (blocks, 1, pupils of the slice); w: pupils x m x n
__global__ __launch_bounds__(kMmBlock) void mmdft_table_kernel(int n, int m, MmdftPads pads,
                                                               double2* __restrict__ w) {
  const double pad = pads.v[blockIdx.z];
  const int64_t cells = (int64_t)m * n;
  double2* out = w + (int64_t)blockIdx.z * cells;
  for (int64_t idx = (int64_t)blockIdx.x * kMmBlock + threadIdx.x; idx < cells;
       idx += (int64_t)gridDim.x * kMmBlock) {
    const int v = (int)(idx / n), j = (int)(idx - (int64_t)v * n);
    const double k = (double)((v - m / 2) * (j - n / 2));  // |k| <= 2^24: exact
    const double t = k / pad;
    const double t_lo = fma(-t, pad, k) / pad;
    double s, c;
    sincospi(2.0 * phase_cycles(t, t_lo), &s, &c);
    out[idx] = make_double2(c, -s);
  }
}

// grid = (blocks, 1, pupils of the slice); count: one zeroed 64-bit word per pupil
__global__ __launch_bounds__(kMmBlock) void mmdft_count_kernel(
    int64_t cells, const double2* __restrict__ pupil, unsigned long long* __restrict__ count) {
  __shared__ unsigned int part[kMmBlock];
  const double2* g = pupil + (int64_t)blockIdx.z * cells;
  unsigned int mine = 0;
  for (int64_t idx = (int64_t)blockIdx.x * kMmBlock + threadIdx.x; idx < cells;
       idx += (int64_t)gridDim.x * kMmBlock) {
    const double2 z = g[idx];
    mine += hypot(z.x, z.y) > 0.0 ? 1u : 0u;  // (a NaN cell compares false)
  }
  part[threadIdx.x] = mine;
  __syncthreads();
  for (int s = kMmBlock / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0 && part[0]) atomicAdd(count + blockIdx.z, (unsigned long long)part[0]);
}

// C[r][c] = sum_k A[r][k] B(k, c) for one 64 x 64 tile of C; grid = (column tiles, row tiles,
// pupils of the slice).  A: rows x depth, the reduction index contiguous.  B: depth x cols with
// the columns contiguous (kBDepthMajor) or cols x depth with the reduction index contiguous.
// kEpilogue: psf = |C|^2 100 / count^2, and C itself only where `c` is given.
template <bool kBDepthMajor, bool kEpilogue>
__global__ __launch_bounds__(kMmBlock) void mmdft_product_kernel(
    int rows, int cols, int depth, const double2* __restrict__ a, int64_t a_pupil,
    const double2* __restrict__ b, int64_t b_pupil, double2* __restrict__ c,
    const unsigned long long* __restrict__ count, double* __restrict__ psf) {
  __shared__ double2 as[kMmDepth][kMmRow];
  __shared__ double2 bs[kMmDepth][kMmRow];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int row0 = blockIdx.y * kMmTile, col0 = blockIdx.x * kMmTile;
  a += (int64_t)blockIdx.z * a_pupil;
  b += (int64_t)blockIdx.z * b_pupil;
  const int64_t out_pupil = (int64_t)blockIdx.z * rows * cols;

  // what this lane moves into the LDS tiles: 4 entries of each (outside the matrices: zero)
  double2 ra[4], rb[4];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int idx = tid + kMmBlock * e;
      const int kk = idx & (kMmDepth - 1), r = idx >> 4;  // depth fastest: 256-byte runs
      const int gr = row0 + r, gk = k0 + kk;
      ra[e] = gr < rows && gk < depth ? a[(int64_t)gr * depth + gk] : make_double2(0.0, 0.0);
      if (kBDepthMajor) {
        const int cc = idx & (kMmTile - 1), kb = idx >> 6;  // columns fastest
        const int gc = col0 + cc, gkb = k0 + kb;
        rb[e] = gc < cols && gkb < depth ? b[(int64_t)gkb * cols + gc] : make_double2(0.0, 0.0);
      } else {
        const int gc = col0 + r;
        rb[e] = gc < cols && gk < depth ? b[(int64_t)gc * depth + gk] : make_double2(0.0, 0.0);
      }
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int idx = tid + kMmBlock * e;
      as[idx & (kMmDepth - 1)][idx >> 4] = ra[e];
      if (kBDepthMajor)
        bs[idx >> 6][idx & (kMmTile - 1)] = rb[e];
      else
        bs[idx & (kMmDepth - 1)][idx >> 4] = rb[e];
    }
  };

  double re[kMmReg][kMmReg], im[kMmReg][kMmReg];
#pragma unroll
  for (int i = 0; i < kMmReg; ++i)
#pragma unroll
    for (int j = 0; j < kMmReg; ++j) re[i][j] = im[i][j] = 0.0;

  // acc += a b as (acc + a.re b) - / + a.im (b.im, b.re): four roundings, each relative to a
  // partial sum -- 2 N roundings of 2^-53 per N-term sum (the bound of tests/_mmdft.py)
  auto step = [&](int kk) {
    double2 av[kMmReg], bv[kMmReg];
#pragma unroll
    for (int i = 0; i < kMmReg; ++i) av[i] = as[kk][ty + 16 * i];  // 16 lanes share an address
#pragma unroll
    for (int j = 0; j < kMmReg; ++j) bv[j] = bs[kk][tx + 16 * j];
#pragma unroll
    for (int i = 0; i < kMmReg; ++i)
#pragma unroll
      for (int j = 0; j < kMmReg; ++j) {
        re[i][j] = fma(-av[i].y, bv[j].y, fma(av[i].x, bv[j].x, re[i][j]));
        im[i][j] = fma(av[i].y, bv[j].x, fma(av[i].x, bv[j].y, im[i][j]));
      }
  };

  fetch(0);
  for (int k0 = 0; k0 < depth; k0 += kMmDepth) {
    stage();
    __syncthreads();
    if (k0 + kMmDepth < depth) fetch(k0 + kMmDepth);
    const int left = depth - k0;
    if (left >= kMmDepth) {
#pragma unroll
      for (int kk = 0; kk < kMmDepth; ++kk) step(kk);
    } else {
      for (int kk = 0; kk < left; ++kk) step(kk);  // (no zero terms: index order, N terms)
    }
    __syncthreads();
  }

  double norm = 0.0;
  if (kEpilogue) {
    const double cnt = (double)count[blockIdx.z];  // <= 2^26: its square is exact
    norm = cnt * cnt;
  }
#pragma unroll
  for (int i = 0; i < kMmReg; ++i) {
    const int gr = row0 + ty + 16 * i;
    if (gr >= rows) continue;
#pragma unroll
    for (int j = 0; j < kMmReg; ++j) {
      const int gc = col0 + tx + 16 * j;
      if (gc >= cols) continue;
      const int64_t o = out_pupil + (int64_t)gr * cols + gc;
      if (!kEpilogue || c) c[o] = make_double2(re[i][j], im[i][j]);
      // mmdft.py:175-177: real(G conj(G)) * 100 / norm; 0 * 100 / 0 = NaN for an empty pupil
      if (kEpilogue) psf[o] = fma(re[i][j], re[i][j], im[i][j] * im[i][j]) * 100.0 / norm;
    }
  }
}

static unsigned blocks_for(int64_t n, int64_t most) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + kMmBlock - 1) / kMmBlock, most));
}

}  // namespace ol

using namespace ol;

extern "C" int ol_mmdft_psf(int32_t n_pupils, int32_t n_side, const double* pupil,
                            const double* pad_size, int32_t image_size, double* psf_out,
                            double* field_out, void* stream) {
  if (n_pupils < 0)
    return failf(OL_EINVAL, "ol_mmdft_psf: negative count (n_pupils %d)", n_pupils);
  if (n_side < 1 || n_side > OL_MMDFT_MAX_SIDE)
    return failf(OL_EINVAL, "ol_mmdft_psf: n_side %d is outside 1..%d", n_side,
                 OL_MMDFT_MAX_SIDE);
  if (image_size < 1 || image_size > OL_MMDFT_MAX_SIDE)
    return failf(OL_EINVAL, "ol_mmdft_psf: image_size %d is outside 1..%d", image_size,
                 OL_MMDFT_MAX_SIDE);
  if (n_pupils == 0) return OL_OK;
  if (!pupil) return failf(OL_EINVAL, "ol_mmdft_psf: pupil is NULL");
  if (!pad_size) return failf(OL_EINVAL, "ol_mmdft_psf: pad_size is NULL");
  if (!psf_out) return failf(OL_EINVAL, "ol_mmdft_psf: psf_out is NULL");
  for (int32_t p = 0; p < n_pupils; ++p)
    if (!(pad_size[p] > 0.0) || std::isinf(pad_size[p]))
      return failf(OL_EINVAL, "ol_mmdft_psf: pad_size[%d] = %g must be finite and positive", p,
                   pad_size[p]);

  hipStream_t st = (hipStream_t)stream;
  const int n = n_side, m = image_size;
  const size_t slice = (size_t)std::min<int32_t>(n_pupils, kSlice);
  const size_t cells = (size_t)n * n, table = (size_t)m * n, pixels = (size_t)m * m;
  const size_t count_bytes = 256;  // kSlice 64-bit words
  static_assert(kSlice * sizeof(unsigned long long) <= 256, "the counts' share of the workspace");
  Workspace ws{"ol_mmdft_psf", st};
  if (int rc = ws.alloc(count_bytes + slice * table * 2 * sizeof(double2))) return rc;
  unsigned long long* count = (unsigned long long*)ws.ptr;
  double2* w = (double2*)((char*)ws.ptr + count_bytes);
  double2* t = w + slice * table;
  const unsigned tiles_n = (unsigned)((n + kMmTile - 1) / kMmTile);
  const unsigned tiles_m = (unsigned)((m + kMmTile - 1) / kMmTile);

  for (int32_t p0 = 0; p0 < n_pupils; p0 += kSlice) {
    const unsigned nb = (unsigned)std::min<int32_t>(n_pupils - p0, kSlice);
    MmdftPads pads;
    for (unsigned p = 0; p < kSlice; ++p) pads.v[p] = p < nb ? pad_size[p0 + p] : 1.0;
    const double2* g = (const double2*)pupil + (size_t)p0 * cells;
    double* psf = psf_out + (size_t)p0 * pixels;
    double2* field = field_out ? (double2*)field_out + (size_t)p0 * pixels : nullptr;
    if (hipMemsetAsync(count, 0, count_bytes, st) != hipSuccess) break;  // (finish() reports it)
    hipLaunchKernelGGL(mmdft_count_kernel, dim3(blocks_for((int64_t)cells, 64), 1, nb),
                       dim3(kMmBlock), 0, st, (int64_t)cells, g, count);
    hipLaunchKernelGGL(mmdft_table_kernel, dim3(blocks_for((int64_t)table, 4096), 1, nb),
                       dim3(kMmBlock), 0, st, n, m, pads, w);
    hipLaunchKernelGGL((mmdft_product_kernel<false, false>), dim3(tiles_m, tiles_n, nb),
                       dim3(kMmBlock), 0, st, n, m, n, g, (int64_t)cells, (const double2*)w,
                       (int64_t)table, t, (const unsigned long long*)nullptr, (double*)nullptr);
    hipLaunchKernelGGL((mmdft_product_kernel<true, true>), dim3(tiles_m, tiles_m, nb),
                       dim3(kMmBlock), 0, st, m, m, n, (const double2*)w, (int64_t)table,
                       (const double2*)t, (int64_t)table, field,
                       (const unsigned long long*)count, psf);
  }
  return ws.finish();
}
