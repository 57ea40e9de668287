// single_surface.h -- what the four one-surface launches share (forbes.hip, grating.hip,
// phase.hip, grid_sag.hip): the kernel arguments, the ray I/O of a lane, the launch shape and the
// tail of the entry point.  The kernels themselves stay in their units, each with its own step,
// launch bounds and status rule.  The entries' argument rules: single_host.h.  Compiles for the
// host under OL_HOST_MATH: the stand-alone programs of tests/host*/ run this ray I/O on host
// buffers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/optiland_hip.h"
#include "single_host.h"
#include "surface_math.h"
#include "trace_launch.h"

namespace ol {

// the table of one precision
template <typename T>
struct Rows {
  const DevSurfHot<T>* hot;
  const DevSurfCold<T>* cold;
  const DevOptics<T>* opt;
  const T* coeffs;
};
template <typename T>
Rows<T> rows_of(const SystemView& v);
template <>
inline Rows<double> rows_of<double>(const SystemView& v) {
  return {v.surf, v.cold, v.optics, v.coeffs};
}
template <>
inline Rows<float> rows_of<float>(const SystemView& v) {
  return {v.surf32, v.cold32, v.optics32, v.coeffs32};
}

// Packed to 4 bytes: no padding behind `flags`, so that what a kernel adds (GratingArgs,
// PhaseArgs) starts right there and every kernel keeps the kernarg layout it has always had.
// Every field sits at its natural alignment all the same.
#pragma pack(push, 4)
template <typename T>
struct SingleArgs {
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
#pragma pack(pop)
static_assert(sizeof(SingleArgs<float>) == 132 && sizeof(SingleArgs<double>) == 132, "");

template <typename T>
SingleArgs<T> single_args(const SystemView& v, int32_t surface, int32_t wl, int64_t n,
                          void* const rays[8], void* row, int64_t stride, uint32_t flags,
                          uint32_t* status) {
  const Rows<T> t = rows_of<T>(v);
  SingleArgs<T> a{};
  a.hot = t.hot + surface;
  a.cold = t.cold + surface;
  a.opt = t.opt + ((int64_t)surface * v.n_wl + wl);
  a.coeffs = t.coeffs;
  for (int k = 0; k < 8; ++k) a.rays[k] = static_cast<T*>(rays[k]);
  a.row = static_cast<T*>(row);
  a.stride = stride;
  a.n = n;
  a.status = status;
  a.flags = flags;
  return a;
}

template <typename T>
OL_DEV Ray<T> single_load(const SingleArgs<T>& a, int64_t i) {
  Ray<T> r;
  r.x = a.rays[0][i]; r.y = a.rays[1][i]; r.z = a.rays[2][i];
  r.L = a.rays[3][i]; r.M = a.rays[4][i]; r.N = a.rays[5][i];
  r.i = a.rays[6][i]; r.opd = a.rays[7][i];
  return r;
}

template <typename T>
OL_DEV SurfFetched<T> single_fetched(const SingleArgs<T>& a) {
  return SurfFetched<T>{as_const(a.hot), as_const(a.cold), as_const(a.opt)};
}

// the recorded row, then the ray state written back
template <typename T>
OL_DEV void single_store(const SingleArgs<T>& a, int64_t i, const Ray<T>& g) {
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
}

constexpr int kSingleThreads = 256;   // the launch bound of the four kernels

// one ray per lane.  Small calls: one wave per workgroup, so that the rays spread over the
// compute units
struct SingleGrid {
  dim3 blocks, threads;
};
inline SingleGrid single_grid(int64_t n) {
  const int block = n >= (int64_t)kSingleThreads * 256 ? kSingleThreads : 64;
  return {dim3((unsigned)((n + block - 1) / block)), dim3(block)};
}

// An entry behind its single_check: `launch(T{}, v, stream)` launches the entry's kernel of
// precision T on the tables of `v`.
template <typename Launch>
int single_entry(const char* who, const ol_system* sys, ol_dtype dt, int64_t n_rays, void* stream,
                 Launch launch) {
  if (n_rays == 0) return OL_OK;
  const SystemView v = system_view(sys);
  if (int rc = rule_current_device(who, v)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (dt == OL_F32)
    launch(float{}, v, st);
  else
    launch(double{}, v, st);
  Workspace ws{who, st};
  return ws.finish();
}

}  // namespace ol
