// gi_kdbuild.h -- photon-map kd-tree built on the device (gi_kdbuild.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gi_dbuf.h"

namespace gi {
// emission-ordered photon record as gi_photon (include/gi.h) / gi_photon_dev: 20 bytes
struct KdPhoton {
  float pos[3];
  uint32_t rgbe;
  uint16_t dir;
  uint16_t flags;
};
static_assert(sizeof(KdPhoton) == 20, "photon record is 20 bytes");

struct KdBuildScratch {
  DBuf perm0, perm1, box;  // uint32_t
  DBuf key0, key1;         // uint64_t
  DBuf axis;               // int32_t
  DBuf tmp;
  hipError_t grow(int64_t n, int64_t L);
};

// Builds the map's implicit kd tree (leaves of <= leaf_size photons; gi_ctx.h HostMap
// layout) from n emission-ordered photons on the device: pos4 (16 B per photon), rgbe and nodes
// (16 * L floats) in kd order, perm_out (host memory, may be null) = kd order -> emission index.
// Asynchronous on st (perm_out is valid after the stream synchronises).
hipError_t kd_build_device(const KdPhoton *ph, int64_t n, int leaf_size, KdBuildScratch &s,
                           float *pos4, uint32_t *rgbe, float *nodes, uint32_t *perm_out,
                           int *nleaves, int *levels, hipStream_t st);
}  // namespace gi
