// ensemble_store.h -- what an ol_ensemble IS on the host: the stacked device tables of both
// precisions, variant 0 as created (what every later variant is held against) and the host images
// of queued copies.  Shared by the translation units that serve an ensemble (ensemble.hip creates,
// updates and destroys it and traces spots; ensemble_opd.hip traces wavefronts) -- the entry points
// of either read the same handle.  Host-only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/optiland_hip.h"
#include "ensemble_device.h"
#include "system_stage.h"
#include "table_image.h"

namespace ol {

// the stacked tables of one precision: ONE allocation, each table on a 256-byte boundary
template <typename T>
struct EnsembleStore {
  char* blob = nullptr;
  EnsembleTables<T> dev{};
};

// the host image of consecutive variants, table by table: what the copies of an upload read
template <typename T>
struct RangeImage {
  std::vector<DevSurfHot<T>> surf;
  std::vector<DevSurfCold<T>> cold;
  std::vector<DevOptics<T>> optics;
  std::vector<T> coeffs;
  std::vector<RaygenConsts<T>> rgc;
};

}  // namespace ol

struct ol_ensemble {
  int32_t n_variants = 0, n_surf = 0, n_wl = 0;
  int device = 0;
  size_t coef_cap = 1;
  int family = 0;                        // Newton kernel family of the shared structure
  bool apod = false;
  // variant 0 as created: what every later variant is held against
  std::vector<ol_surface_desc> ref_rows;
  int32_t ref_coeffs = 0;
  ol_raygen_params ref_raygen{};
  ol::Staged ref;
  ol::EnsembleStore<float> f32;
  ol::EnsembleStore<double> f64;
  bool consistent = true;   // false between the two uploads of an update, for good if one fails
  // The sources of the queued copies.  They are pageable memory, megabytes of it at thousands of
  // variants, and nothing here leans on when the runtime has finished reading such a source: the
  // images live in the ensemble, `copied` is recorded behind the copies, and the next update
  // (or the destruction) waits for it before the images are written again (or freed).
  ol::RangeImage<float> image32;
  ol::RangeImage<double> image64;
  hipEvent_t copied = nullptr;
};
