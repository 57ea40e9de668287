// last_error.h -- what the host side of every translation unit shares: the library's one
// thread-local error message (ol_last_error) and the stream-ordered workspace of an entry point.
// failf is defined in capi.hip; capi.hip itself references no symbol of the other units
// (tests/hostmath links it alone).  The argument rules the entry points share, and their texts,
// are stated once in entry_rules.h, which builds on this header and on system_view.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

#include "../../include/optiland_hip.h"
#include "failf.h"

namespace ol {

// Scratch memory of one entry point, allocated and freed in stream order:
//   Workspace ws{"ol_x", stream};  if (int rc = ws.alloc(bytes)) return rc;
//   ... launches ...               return ws.finish();
// An entry point without scratch memory calls finish() alone.
struct Workspace {
  const char* who;
  hipStream_t stream;
  void* ptr = nullptr;

  int alloc(size_t bytes) {  // 0 bytes: no allocation, ptr stays NULL
    if (bytes == 0) return OL_OK;
    const hipError_t e = hipMallocAsync(&ptr, bytes, stream);
    if (e == hipSuccess) return OL_OK;
    return failf(e == hipErrorOutOfMemory ? OL_ENOMEM : OL_EHIP,
                 "%s: workspace of %zu bytes: %s", who, bytes, hipGetErrorString(e));
  }
  int finish() {  // after the last launch: the first error of the launches and of the free
    hipError_t e = hipGetLastError();
    if (ptr) {
      const hipError_t f = hipFreeAsync(ptr, stream);
      if (e == hipSuccess) e = f;
    }
    if (e != hipSuccess) return failf(OL_EHIP, "%s: launch failed: %s", who, hipGetErrorString(e));
    return OL_OK;
  }
};

}  // namespace ol
