// gi_sort.h -- Morton ordering of query batches (gi_sort.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gi_dbuf.h"

namespace gi {
struct SortScratch {
  DBuf k0, k1, v0, v1, tmp;
  DBuf rows, cnt;  // curve_order_rows: the row masks and their counts / offsets
};
// returns a device permutation (sorted position -> query index) valid until the next call
hipError_t morton_order(const float4 *q, int64_t n, const float bmin[3], const float bmax[3],
                        SortScratch &s, uint32_t **perm_out, hipStream_t st);
// the same with the empty slots (meta == QMETA_NONE) sorted after every valid query: the first
// *nvalid entries of the permutation are the valid queries in morton_order's order, so the k-NN
// launch takes only those (synchronises st for the count)
// key_bits > 10: cells of key_bits (<= 20) bits per axis and 64-bit keys; with surf as well, 64-bit
// surface keys with 16-bit in-plane cells (gi_sort.hip surf64_valid_kernel)
hipError_t morton_order_valid(const float4 *q, int64_t n, const float bmin[3], const float bmax[3],
                              SortScratch &s, uint32_t **perm_out, int64_t *nvalid, hipStream_t st,
                              int key_bits = 10, bool surf = false, uint32_t qbase = 0,
                              const uint32_t *app_order = nullptr);
// qbase, app_order (both sorts; null: slot order): the slots [qbase, n) are a render list's Monte
// Carlo appends, which take their slots in arrival order; they enter the sort in the order
// app_order gives (key_order's sslots of their own keys, relative to qbase), so that queries with
// equal sort keys come out in the same order in every launch
// The global list's launch order built from its slot layout instead of a sort over every slot:
// primary slots [0, nprim) (validity read from q), then the tiled indirect slots [nprim,
// nprim + 64 trows) whose row masks qmask[r] mark the entries holding a query (the reduction's
// own masks, gi_kernels.hip ind_kernel / ind_cont_kernel), then the appends [qbase, nq), all
// valid. The valid slots are compacted (row popcounts, a scan, a scatter: no per-slot pass over
// the empty ones), keyed like morton_order_valid and sorted: the first *nvalid entries of the
// permutation are the same queries, in the same order, as morton_order_valid's. With surf the
// keys are surface keys instead (gi_sort.hip surface_key: the face of the query's normal, a
// depth slab, the 2-D Hilbert curve in the face's plane).
hipError_t curve_order_rows(const float4 *q, int64_t nprim, const uint64_t *qmask, int64_t trows,
                            uint32_t qbase, int64_t nq, const float bmin[3], const float bmax[3],
                            SortScratch &s, uint32_t **perm_out, int64_t *nvalid, hipStream_t st,
                            bool surf = false, const uint32_t *app_order = nullptr);
// key parameters: the 3-D curve's 10-bit cells (origin o, scale s per axis, cmax), or, with surf,
// the surface key's square 11-bit cells (siso) and 32 depth slabs per axis (sdep)
struct KeyGeom {
  float o[3], s[3], cmax;
  float siso, sdep[3];
  int surf;
};

struct KeySortScratch {
  DBuf k1, v0, v1, tmp;
};
// stable order of 64-bit keys: sorted keys + the original slot of each
hipError_t key_order(const uint64_t *keys, int64_t n, int key_bits, KeySortScratch &s,
                     uint64_t **skeys, uint32_t **sslots, hipStream_t st);
}  // namespace gi
